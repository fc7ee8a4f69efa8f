// Host side of the ptk C-ABI: the multi-GPU exchange step - packed layout, the context's own RCCL communicator, the gather of every
// rank's owned tiles to the root, and the parity probes of its two kernels (ptk.h).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <thread>
#include <type_traits>

#include "ptk_ctx.h"
#include "ptk_stage.h"
#include "ptk_device_fn.h"

using namespace ptk;
static_assert(std::is_same<ncclComm_t, struct ncclComm*>::value, "ptk_ctx.h repeats rccl.h's ncclComm_t: keep the two alike");

void ptk::comm_release(ptk_ctx* c)
{
    if (c->comm) { (void)ncclCommDestroy(c->comm); c->comm = nullptr; }
}

extern "C" {

static int64_t packed_floats_of(int width, int height, int rank, int world)
{
    const int64_t tiles = (int64_t)((width + PTK_TILE - 1) / PTK_TILE) * ((height + PTK_TILE - 1) / PTK_TILE);
    const int64_t owned = tiles <= rank ? 0 : (tiles - rank + world - 1) / world;
    return owned * PTK_TILE * PTK_TILE * 3;
}

int64_t ptk_packed_floats(int width, int height, int rank, int world)
{
    if (width <= 0 || height <= 0 || world < 1 || rank < 0 || rank >= world) return -1;
    return packed_floats_of(width, height, rank, world);
}

int ptk_packed_layout(int width, int height, int rank, int world, int64_t* src_index)
{
    if (width <= 0 || height <= 0 || world < 1 || rank < 0 || rank >= world || !src_index) return PTK_ERR_BAD_ARG;
    const int tiles_x = (width + PTK_TILE - 1) / PTK_TILE, num_tiles = tiles_x * ((height + PTK_TILE - 1) / PTK_TILE);
    int64_t k = 0;
    for (int tile = rank; tile < num_tiles; tile += world)
    {
        int tx, ty; tile_origin(tile, tiles_x, tx, ty);
        for (int p = 0; p < PTK_TILE * PTK_TILE; p++)
        {
            const int px = tx * PTK_TILE + (p & 15), py = ty * PTK_TILE + (p >> 4);
            const bool on = px < width && py < height;
            const int64_t a = ((int64_t)(height - 1 - py) * width + px) * 3;
            for (int ch = 0; ch < 3; ch++) src_index[k++] = on ? a + ch : -1;
        }
    }
    return PTK_OK;
}

int ptk_comm_unique_id(void* id_out)
{
    if (!id_out) return PTK_ERR_BAD_ARG;
    static_assert(sizeof(ncclUniqueId) == 128, "ptk.h promises 128 bytes");
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return PTK_ERR_RCCL;
    std::memcpy(id_out, &id, sizeof(id));
    return PTK_OK;
}

int ptk_comm_init(ptk_ctx* c, const void* id_in, int rank, int world)
{
    if (!c || !id_in || world < 1 || world > PTK_MAX_RANKS || rank < 0 || rank >= world) return PTK_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    comm_release(c);
    // ncclCommInitRank blocks until EVERY rank of the group has called it: a rank that died on the way (or was never started)
    // would hang the others for good.  It runs on a helper thread and is waited for with a bound; on a timeout the caller gets an
    // error that names the rank and is expected to end the process (the helper thread is abandoned with its own state).
    struct InitJob { ncclComm_t comm = nullptr; ncclResult_t r = ncclSuccess; std::atomic<int> done{ 0 }; };
    auto job = std::make_shared<InitJob>();
    ncclUniqueId id;
    std::memcpy(&id, id_in, sizeof(id));
    const int device = c->device;
    std::thread([job, id, rank, world, device] {
        (void)hipSetDevice(device);
        job->r = ncclCommInitRank(&job->comm, world, id, rank);
        job->done.store(1);
    }).detach();
    const auto t0 = std::chrono::steady_clock::now();
    while (!job->done.load())
    {
        const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (waited > c->opt_comm_timeout_s)
        {
            char msg[256];
            std::snprintf(msg, sizeof(msg), "ncclCommInitRank: rank %d of %d (HIP device %d) waited %.0f s for the other ranks to join the communicator - "
                          "is every rank running, on a device of its own?", rank, world, device, waited);
            return fail(c, PTK_ERR_RCCL, msg);
        }
        std::this_thread::sleep_for(std::chrono::milliseconds(2));
    }
    if (job->r != ncclSuccess || !job->comm)
    {
        char msg[256];
        std::snprintf(msg, sizeof(msg), "ncclCommInitRank: rank %d of %d (HIP device %d): %s", rank, world, device, ncclGetErrorString(job->r));
        return fail(c, PTK_ERR_RCCL, msg);
    }
    c->comm = job->comm;
    c->comm_rank = rank; c->comm_world = world;
    c->rank = rank; c->world = world;            // the frame is split over the group (ptk_set_tile)
    return PTK_OK;
}

int ptk_comm_info(ptk_ctx* c, int* rank, int* world, int* comm_device, int* ctx_device)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (ctx_device) *ctx_device = c->device;
    if (!c->comm) return fail(c, PTK_ERR_BAD_ARG, "no communicator: call ptk_comm_init");
    int r = -1, w = 0, d = -1;
    if (ncclCommCount(c->comm, &w) != ncclSuccess || ncclCommUserRank(c->comm, &r) != ncclSuccess || ncclCommCuDevice(c->comm, &d) != ncclSuccess)
        return fail(c, PTK_ERR_RCCL, "ncclCommCount / ncclCommUserRank / ncclCommCuDevice failed");
    if (rank) *rank = r;
    if (world) *world = w;
    if (comm_device) *comm_device = d;
    return PTK_OK;
}

int ptk_comm_destroy(ptk_ctx* c)
{
    if (!c) return PTK_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    if (c->xstream) (void)hipStreamSynchronize(c->xstream);
    comm_release(c);
    return PTK_OK;
}

// Packed gather.  Everything is queued on the context's exchange stream behind what the render stream holds now:
//   pack kernel (snapshot of the owned tiles; the render stream waits only for this) -> grouped ncclSend / ncclRecv
//   (each rank's 1/world of the image goes straight to the root over its own xGMI link) -> root: unpack kernel.
// The next ptk_render may be issued at once: its trace kernel does not touch the accumulator and overlaps the exchange.
int ptk_gather_accum(ptk_ctx* c, void* rccl_comm, int root)
{
    if (!c) return PTK_ERR_BAD_ARG;
    ncclComm_t comm = rccl_comm ? (ncclComm_t)rccl_comm : c->comm;
    if (!comm) return fail(c, PTK_ERR_BAD_ARG, "no communicator: pass one or call ptk_comm_init");
    if (!accum_ptr(c)) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    int world = 0, rank = 0;
    if (ncclCommCount(comm, &world) != ncclSuccess || ncclCommUserRank(comm, &rank) != ncclSuccess)
        return fail(c, PTK_ERR_RCCL, "ncclCommCount / ncclCommUserRank failed");
    if (world != c->world || rank != c->rank) return fail(c, PTK_ERR_BAD_ARG, "communicator rank / size differ from ptk_set_tile");
    if (root < 0 || root >= world || world > PTK_MAX_RANKS) return fail(c, PTK_ERR_BAD_ARG, "bad root");
    const int W = c->width, H = c->height;
    long long bases[PTK_MAX_RANKS] = { 0 };
    size_t total = 0;
    for (int r = 0; r < world; r++) { bases[r] = (long long)total; total += (size_t)packed_floats_of(W, H, r, world); }
    const size_t mine = (size_t)packed_floats_of(W, H, rank, world);
    const size_t need = rank == root ? total : mine;
    int rg = c->d_packed.grow(c, need, sizeof(float), 0, c->xstream);
    if (rg == PTK_OK && rank == root) rg = c->d_gathered.grow(c, (size_t)W * H * 3, sizeof(float), 0, c->xstream);
    if (rg != PTK_OK) return rg;
    HIPCHK(c, hipEventRecord(c->ev_rendered, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->xstream, c->ev_rendered, 0));
    float* my_slot = c->d_packed + (rank == root ? bases[rank] : 0);
    launch_pack_owned(accum_ptr(c), my_slot, W, H, rank, world, c->xstream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_packed, c->xstream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_packed, 0));      // the next accumulate_kernel may overwrite the accumulator from here on
    if (world > 1)
    {
        ncclResult_t r = ncclGroupStart();
        if (r == ncclSuccess)
        {
            if (rank == root)
            {
                for (int src = 0; src < world && r == ncclSuccess; src++)
                {
                    const size_t n = (size_t)packed_floats_of(W, H, src, world);
                    if (src != root && n) r = ncclRecv(c->d_packed + bases[src], n, ncclFloat, src, comm, c->xstream);
                }
            }
            else if (mine) r = ncclSend(my_slot, mine, ncclFloat, root, comm, c->xstream);
            ncclResult_t e = ncclGroupEnd();
            if (r == ncclSuccess) r = e;
        }
        if (r != ncclSuccess) return fail(c, PTK_ERR_RCCL, std::string("packed gather (ncclSend/ncclRecv): ") + ncclGetErrorString(r));
    }
    if (rank == root)
    {
        launch_unpack_all(c->d_packed, bases, c->d_gathered, W, H, world, c->xstream);
        HIPCHK(c, hipGetLastError());
        c->gathered_w = W; c->gathered_h = H;
    }
    HIPCHK(c, hipEventRecord(c->ev_gathered, c->xstream));
    c->gather_pending = true;
    c->gather_step++; c->gather_root = root;
    c->gather_bytes = (rank == root ? total - mine : mine) * sizeof(float);
    return PTK_OK;
}

// Bounded: polls the exchange's last event; when it has not fired within comm_timeout_s (a rank never entered its
// ptk_gather_accum, or died in it) the communicator is aborted - which releases the transfer kernel stuck on the exchange
// stream - and the caller gets PTK_ERR_RCCL with rank, step and the bytes that were expected.  An asynchronous RCCL error
// (a peer's process gone) ends the wait at once.  A failed exchange leaves no gathered image: d_gathered may hold part of this
// step's or the last step's image, so ptk_read_gathered and ptk_gathered_device_ptr refuse until a ptk_gather_accum succeeds.
int ptk_gather_wait(ptk_ctx* c)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!c->gather_pending) return PTK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    for (;;)
    {
        const hipError_t q = hipEventQuery(c->ev_gathered);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady)
        {
            c->gather_pending = false; c->gathered_w = c->gathered_h = 0;
            return fail(c, PTK_ERR_HIP, std::string("hipEventQuery (exchange): ") + hipGetErrorString(q));
        }
        (void)hipGetLastError();
        const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        ncclResult_t async = ncclSuccess;
        const bool poll_comm = c->comm && (++spins & 1023u) == 0;
        if (poll_comm && ncclCommGetAsyncError(c->comm, &async) != ncclSuccess) async = ncclSystemError;
        if (waited > c->opt_comm_timeout_s || (async != ncclSuccess && async != ncclInProgress))
        {
            char msg[384];
            std::snprintf(msg, sizeof(msg), "exchange step %llu on rank %d of %d (root %d) %s after %.1f s: %s %zu bytes%s",
                          c->gather_step, c->rank, c->world, c->gather_root,
                          async != ncclSuccess && async != ncclInProgress ? "failed" : "timed out", waited,
                          c->rank == c->gather_root ? "still expecting" : "still sending", c->gather_bytes,
                          async != ncclSuccess && async != ncclInProgress ? (std::string(" - RCCL: ") + ncclGetErrorString(async)).c_str() : " - a rank never joined this step");
            if (c->comm)
            {
                // the abort releases RCCL's own kernels, but it also waits for whatever else sits on the stream: it runs on a helper
                // thread and this call gives it one more timeout's worth (at most 5 s) before it returns regardless
                ncclComm_t doomed = c->comm;
                c->comm = nullptr;
                auto done = std::make_shared<std::atomic<bool>>(false);
                std::thread([doomed, done] { (void)ncclCommAbort(doomed); done->store(true); }).detach();
                const auto a0 = std::chrono::steady_clock::now();
                const double grace = std::min(c->opt_comm_timeout_s, 5.0);
                while (!done->load() && std::chrono::duration<double>(std::chrono::steady_clock::now() - a0).count() < grace)
                    std::this_thread::sleep_for(std::chrono::milliseconds(1));
            }
            c->gather_pending = false; c->gathered_w = c->gathered_h = 0;
            return fail(c, PTK_ERR_RCCL, msg);
        }
        if (waited > 0.002) std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    c->gather_pending = false;
    return PTK_OK;
}

// Test hook of the bounded waits: one lane that keeps the exchange stream busy for a fixed time (wall clock, 100 MHz), so that
// a single GPU can show what ptk_gather_wait does when an exchange step does not complete in time.  It always ends by itself.
__global__ void stall_kernel(unsigned long long ticks)
{
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}

int ptk_debug_stall_exchange(ptk_ctx* c, int milliseconds)
{
    if (!c || milliseconds < 0 || milliseconds > 10000) return PTK_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    stall_kernel<<<1, 1, 0, c->xstream>>>((unsigned long long)milliseconds * 100000ull);
    HIPCHK(c, hipGetLastError());
    return PTK_OK;
}

int ptk_gathered_device_ptr(ptk_ctx* c, void** dev_ptr, size_t* bytes)
{
    if (!c || !dev_ptr) return PTK_ERR_BAD_ARG;
    *dev_ptr = nullptr;
    if (bytes) *bytes = 0;
    if (!c->d_gathered || c->gathered_w == 0) return fail(c, PTK_ERR_BAD_ARG, "no gathered image on this rank (not the root, or ptk_gather_accum not called)");
    if (c->gathered_w != c->width || c->gathered_h != c->height)
        return fail(c, PTK_ERR_BAD_ARG, "the gathered image was combined for another resolution: call ptk_gather_accum again after ptk_set_frame");
    *dev_ptr = c->d_gathered;
    if (bytes) *bytes = (size_t)c->gathered_w * c->gathered_h * 3 * sizeof(float);
    return PTK_OK;
}

int ptk_read_gathered(ptk_ctx* c, float* host_out)
{
    if (!c || !host_out) return PTK_ERR_BAD_ARG;
    if (!c->d_gathered || c->gathered_w == 0) return fail(c, PTK_ERR_BAD_ARG, "no gathered image on this rank (not the root, or ptk_gather_accum not called)");
    if (c->gathered_w != c->width || c->gathered_h != c->height)
        return fail(c, PTK_ERR_BAD_ARG, "the gathered image was combined for another resolution: call ptk_gather_accum again after ptk_set_frame");
    int rc = ptk_gather_wait(c);
    if (rc != PTK_OK) return rc;
    HIPCHK(c, hipMemcpy(host_out, c->d_gathered, (size_t)c->width * c->height * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return PTK_OK;
}

// parity probes of the two exchange kernels (one GPU can play every rank of a split)
int ptk_probe_pack(ptk_ctx* c, int rank, int world, float* host_out)
{
    if (!c || !host_out || world < 1 || world > PTK_MAX_RANKS || rank < 0 || rank >= world) return PTK_ERR_BAD_ARG;
    if (!accum_ptr(c)) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)packed_floats_of(c->width, c->height, rank, world);
    if (n == 0) return PTK_OK;
    Stage s(c);
    const auto d = s.out(host_out, n);
    return s.run([&] {
        launch_pack_owned(accum_ptr(c), d, c->width, c->height, rank, world, c->stream);
        return s.launched();
    });
}

int ptk_probe_unpack(ptk_ctx* c, int world, const float* host_packed, float* host_image)
{
    if (!c || !host_packed || !host_image || world < 1 || world > PTK_MAX_RANKS) return PTK_ERR_BAD_ARG;
    if (c->width <= 0) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    long long bases[PTK_MAX_RANKS] = { 0 };
    size_t total = 0;
    for (int r = 0; r < world; r++) { bases[r] = (long long)total; total += (size_t)packed_floats_of(c->width, c->height, r, world); }
    const size_t img = (size_t)c->width * c->height * 3;
    Stage s(c);
    const auto d = s.in(host_packed, total), di = s.out(host_image, img);
    return s.run([&] {
        if (hipMemsetAsync(di, 0xff, img * sizeof(float), c->stream) != hipSuccess) return s.launched();      // NaNs: every pixel must be written
        launch_unpack_all(d, bases, di, c->width, c->height, world, c->stream);
        return s.launched();
    });
}

}  // extern "C"
