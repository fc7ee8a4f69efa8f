// Host-side check of the pair pass's accept in the form the kernel runs it (pbrpathtracer_amd/csrc/ptk_flat_mt.h): mt_rect_accept_once -
// one update per ray, hit = X & (inA | inB), first = inA - against mt_rect_accept, the stated sequential rule (A, then B against the best
// A left), which tests/cpp/flat_rect_fuzz.cpp holds to the pass itself.  The two must agree exactly: hit == okA | okB, and first == okA
// whenever hit.
// Directed: the full cross product, over the nine float inputs, of fifteen values - +-0, the smallest denormal of either sign, +-eps,
// the two neighbours of eps, 1 and its two neighbours, +-infinity, a NaN of either sign.  It holds t == best_t, t == eps, |a| == eps,
// uv == 1, a point inside both A and B, u = -0 and a NaN in any place, each beside every value of every other input (15^9 = 3.8e10
// cases over a few threads, only mismatches and accepts counted: seconds; the first seven values' product once more with every tally).
// Random: draws of all nine inputs from raw bit patterns, from the fifteen values and from their near neighbourhood.
//   g++ -O2 -std=c++17 -ffp-contract=off -pthread -I pbrpathtracer_amd/csrc tests/cpp/flat_rect_accept_fuzz.cpp -o f && ./f [values per input] [random draws]
// values per input < 15 takes the first so many of the set (the sanitizer build runs a smaller product); exit status 0 = no mismatch
// and every case named above was met.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

#include "ptk_flat_mt.h"

namespace {

const float EPS = 0.00001f;             // PTK_EPS

inline float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
inline uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

struct Tally
{
    long long cases = 0, bad = 0, hits = 0, first = 0, second = 0, both_in = 0, tie = 0, nan_in = 0, nan_hit = 0;
    void add(const Tally& o)
    {
        cases += o.cases; bad += o.bad; hits += o.hits; first += o.first; second += o.second; both_in += o.both_in; tie += o.tie;
        nan_in += o.nan_in; nan_hit += o.nan_hit;
    }
};

// one case through both functions
inline void one(float a, float t, float uA, float vA, float uvA, float uB, float vB, float uvB, float best, Tally& T)
{
    bool okA, okB, hit, first;
    ptk_mt::mt_rect_accept(a, t, uA, vA, uvA, uB, vB, uvB, best, EPS, okA, okB);
    ptk_mt::mt_rect_accept_once(a, t, uA, vA, uvA, uB, vB, uvB, best, EPS, hit, first);
    const bool wrong = hit != (okA | okB) || (hit && first != okA) || (okA && okB);
    T.cases++;
    if (wrong && T.bad++ < 5)
        std::printf("a %a t %a best %a A (%a %a %a) B (%a %a %a): sequential %d %d, once hit %d first %d\n", a, t, best, uA, vA, uvA, uB, vB, uvB, okA, okB, hit, first);
    T.hits += hit; T.first += okA; T.second += okB;
    T.both_in += hit && first && !(uB < 0.0f) && !(vB < 0.0f) && !(uvB > 1.0f);
    T.tie += t == best;
    const bool any_nan = a != a || t != t || best != best || uA != uA || vA != vA || uvA != uvA || uB != uB || vB != vB || uvB != uvB;
    T.nan_in += any_nan; T.nan_hit += any_nan && hit;
}

std::vector<float> directed()
{
    const float inf = std::numeric_limits<float>::infinity(), den = std::numeric_limits<float>::denorm_min();
    // (a shorter prefix of the set still crosses every threshold: its first seven hold eps and a t above it, 1, zeros, a negative, a NaN)
    return { EPS, 1.0f, from_bits(0x7fc00000u), 0.0f, -0.0f, std::nextafter(EPS, inf), -EPS, std::nextafter(1.0f, inf),
             std::nextafter(1.0f, 0.0f), std::nextafter(EPS, 0.0f), den, -den, inf, -inf, from_bits(0xffc00000u) };
}

// The full product, lean: both functions per case, mismatches and accepts counted, nothing else - the inner loops then keep only what
// their own inputs change.  Work items are (a, t) pairs handed out by a shared counter.
struct Lean { long long cases = 0, bad = 0, hits = 0, first = 0, second = 0; };

void cross(const std::vector<float>& V, std::atomic<size_t>& next_item, Lean& out)
{
    const size_t n = V.size();
    Lean L;
    for (size_t item = next_item++; item < n * n; item = next_item++)
    {
        const float a = V[item / n], t = V[item % n];
        for (float best : V)
            for (float uA : V) for (float vA : V) for (float uvA : V)
                for (float uB : V) for (float vB : V)
                {
                    unsigned bad = 0, hits = 0, first = 0, second = 0;
                    for (float uvB : V)
                    {
                        bool okA, okB, hit, fst;
                        ptk_mt::mt_rect_accept(a, t, uA, vA, uvA, uB, vB, uvB, best, EPS, okA, okB);
                        ptk_mt::mt_rect_accept_once(a, t, uA, vA, uvA, uB, vB, uvB, best, EPS, hit, fst);
                        bad += (hit != (okA | okB)) | (hit & (fst != okA)) | (okA & okB);
                        hits += hit; first += okA; second += okB;
                    }
                    if (bad && L.bad < 5)
                        for (float uvB : V) { Tally T; one(a, t, uA, vA, uvA, uB, vB, uvB, best, T); }       // (prints the cases that differ)
                    L.bad += bad; L.hits += hits; L.first += first; L.second += second; L.cases += (long long)n;
                }
    }
    out = L;
}

// ... and the product of the set's first `n` values with every tally, which shows that the named cases are among them
void cross_tallied(const std::vector<float>& all, size_t n, Tally& T)
{
    const std::vector<float> V(all.begin(), all.begin() + n);
    for (float a : V) for (float t : V) for (float best : V)
        for (float uA : V) for (float vA : V) for (float uvA : V)
            for (float uB : V) for (float vB : V) for (float uvB : V)
                one(a, t, uA, vA, uvA, uB, vB, uvB, best, T);
}

struct Rand
{
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 32); }
    float value(const std::vector<float>& V)
    {
        switch (next() & 3u)
        {
            case 0: return from_bits(next());                                            // any bit pattern: NaNs, denormals, huge
            case 1: return V[next() % V.size()];
            case 2: { const float f = V[next() % V.size()]; return f != f ? f : from_bits(bits(f) + (next() % 5u) - 2u); }      // within two ulps of a directed value
            default: return (float)(next() >> 8) * 5.9604644775390625e-8f * 1.25f - 0.125f;         // [-0.125, 1.125): barycentrics about the edges
        }
    }
};

}  // namespace

int main(int argc, char** argv)
{
    std::vector<float> V = directed();
    const size_t full = V.size();
    const size_t n = argc > 1 ? (size_t)std::atol(argv[1]) : full;
    const long draws = argc > 2 ? std::atol(argv[2]) : 4000000;
    if (n < 3 || n > full) { std::printf("values per input: 3..%zu\n", full); return 4; }
    V.resize(n);
    int status = 0;

    const size_t threads = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    std::vector<Lean> part(threads);
    std::vector<std::thread> pool;
    std::atomic<size_t> next_item{ 0 };
    for (size_t k = 0; k < threads; k++) pool.emplace_back(cross, std::cref(V), std::ref(next_item), std::ref(part[k]));
    for (auto& th : pool) th.join();
    Lean D;
    for (const Lean& p : part) { D.cases += p.cases; D.bad += p.bad; D.hits += p.hits; D.first += p.first; D.second += p.second; }
    long long want = 1;
    for (int k = 0; k < 9; k++) want *= (long long)n;
    std::printf("directed: %zu values per input, %lld cases, hits %lld (A %lld, B %lld); mismatches %lld\n", n, D.cases, D.hits, D.first, D.second, D.bad);
    if (D.bad) status = 1;
    if (D.cases != want || D.first == 0 || D.second == 0 || D.hits != D.first + D.second)
    { std::printf("  the directed product does not reach its cases\n"); status = status ? status : 2; }
    Tally S;
    cross_tallied(V, std::min<size_t>(n, 7), S);
    std::printf("its first values, tallied: %lld cases, hits %lld (A %lld, B %lld), inside both %lld, t == best %lld, with a NaN %lld (accepted %lld); mismatches %lld\n",
                S.cases, S.hits, S.first, S.second, S.both_in, S.tie, S.nan_in, S.nan_hit, S.bad);
    if (S.bad) status = 1;
    if (S.first == 0 || S.second == 0 || S.both_in == 0 || S.tie == 0 || S.nan_in == 0)
    { std::printf("  the directed values do not reach the named cases\n"); status = status ? status : 2; }

    Tally R;
    Rand G{ 2024u };
    const std::vector<float> all = directed();
    for (long k = 0; k < draws; k++)
    {
        const float a = G.value(all), t = G.value(all), uA = G.value(all), vA = G.value(all), uB = G.value(all), vB = G.value(all);
        // uv mostly as the kernel forms it, sometimes a value of its own
        const float uvA = (G.next() & 3u) ? uA + vA : G.value(all), uvB = (G.next() & 3u) ? uB + vB : G.value(all);
        const float best = (G.next() & 3u) == 0u ? t : G.value(all);
        one(a, t, uA, vA, uvA, uB, vB, uvB, best, R);
    }
    std::printf("random: %lld draws, hits %lld (A %lld, B %lld), inside both %lld, t == best %lld, with a NaN %lld (accepted %lld); mismatches %lld\n",
                R.cases, R.hits, R.first, R.second, R.both_in, R.tie, R.nan_in, R.nan_hit, R.bad);
    if (R.bad) status = 1;
    if (draws >= 100000 && (R.first < draws / 2000 || R.second < draws / 2000 || R.both_in == 0 || R.tie < draws / 8 || R.nan_in < draws / 8))
    { std::printf("  the random draws do not reach their cases\n"); status = status ? status : 2; }

    std::printf(status ? "FAILED (%d)\n" : "ok\n", status);
    return status;
}
