"""Headless driver: render a reference `.pts` scene file on the GPU and export a PNG.

    python -m pbrpathtracer_amd.render scene.pts --spp 256 --out image.png [--seed S] [--device D]
    python -m pbrpathtracer_amd.render scene.pts --noise-threshold 0.02 [--min-spp 16] [--step 8] --spp 1024
    python -m pbrpathtracer_amd.render scene.pts --spp 8 --denoise [--denoise-iterations K] [--npy denoised.npy]
    python -m pbrpathtracer_amd.render scene.pts --orbit FRAMES --orbit-degrees D --spp K --temporal [--denoise]
    python -m pbrpathtracer_amd.render scene.pts --orbit FRAMES --spp K --temporal --move-object OBJ --move-by DX DY DZ
    python -m pbrpathtracer_amd.render scene.pts --orbit FRAMES --spp K --temporal --denoise --temporal-variance
                                                 [--motion-vectors FILE.npy]
    python -m pbrpathtracer_amd.render scene.pts ... --display {linear,reinhard,aces} [--exposure auto|EV] [--key K] [--adapt A]
                                                 [--linear-transfer]
    python -m pbrpathtracer_amd.render scene.pts --features planes.npz
    python -m pbrpathtracer_amd.render scene.pts --equirect 2048 --spp 64 [--denoise] -o pano.png [--npy pano.npy]
    python -m pbrpathtracer_amd.render scene.pts --equirect 2048 --hits planes.npz [--layers K] [--attributes]
    python -m pbrpathtracer_amd.render scene.pts --distance-field 64 64 64 [--df-max-dist M] [--signed [--inside-mode parity]] -o field.npz
    python -m pbrpathtracer_amd.render scene.pts --distance-field 64 64 64 --nearest 4 [--df-max-dist M] -o nearest.npz
    python -m pbrpathtracer_amd.render scene.pts --voxelize 64 64 64 [--solid] -o grid.npz
    python -m pbrpathtracer_amd.render scene.pts --point-cloud 100000 --spp 16 [--offset O] -o cloud.npz
    python -m pbrpathtracer_amd.render scene.pts --bake-lightmap 1024 --spp 64 [--bake-atlas] [--bake-offset F] [--bake-back]
                                                 [--denoise] [--dilate K] -o map.png [--npy map.npy]
    python -m pbrpathtracer_amd.render scene.pts --bake-probes NX NY NZ [--probe-dirs D] --spp N -o probes.npz
                                                 [--probe-visibility RES [--probe-max-dist M]]

With --display the PNG of a perspective frame or an --orbit is the frame after the display transform (include/ptk.h
ptk_display_frame, PathTracer.DisplayFrame): an exposure - metered from the frame's luminance histogram, or 2^EV -, the tone curve
named, and the sRGB transfer function (--linear-transfer: none), over the --denoise or --temporal result where there is one.  With
--orbit every step is displayed, so the exposure state on the device adapts from step to step (--adapt below 1 lets it lag).
Without --display every output stays what it is: the plain clamp-and-truncate resolve.

With --noise-threshold the render is adaptive (include/ptk.h ptk_render_adaptive): --spp becomes the most samples a pixel
gets, and pixels stop once their noise meets the threshold.  --equirect and --bake-lightmap take it too (ptk_trace_rays_adaptive,
ptk_bake_lightmap_adaptive): the image is then the mean sum / count per pixel or texel, --npy FILE.npy holds that float32 mean and
FILE.counts.npy beside it the uint32 sample counts.

With --denoise the PNG is the frame after the a-trous denoiser (include/ptk.h ptk_denoise_frame, PathTracer.DenoiseFrame with
ptk.denoise_defaults for the scene's extent; --denoise-iterations overrides the 5 iterations), guided by the first-hit normal,
position and albedo planes - after an adaptive render (--noise-threshold) also by each pixel's variance - and --npy FILE.npy holds
the denoised float32 image [H, W, 3], rows top-down like the PNG.  With --bake-lightmap it filters the baked mean over the covered
texels (lightmap.denoise, guided by the texels' positions and shading normals and demodulated by their albedo: lightmap.guides,
include/ptk.h ptk_surface_attributes) before --dilate pads the charts.  With --equirect it filters the panorama's sums over the
samples (Context.denoise_planes), guided by what the panorama's rays hit (rays.hit_guides: ptk_intersect_rays, then
ptk_surface_attributes for position, shading normal and albedo); --npy then holds the filtered sums.

With --orbit FRAMES the loaded camera is turned about the vertical axis through the centre of the scene's bounds, by --orbit-degrees
in FRAMES equal steps - an interactive session's camera drag.  At each step the image is reset and --spp samples are rendered; with
--temporal each step ends in PathTracer.TemporalFrame (include/ptk.h ptk_temporal_frame, ptk.temporal_defaults for the scene's
extent), which carries the steps before it into the new view.  The PNG is the last view: the reprojected frame - after --denoise
filtered by Context.denoise_planes with the guide planes TemporalFrame rendered - or, without --temporal, the plain last frame of
--spp samples, for comparison.  --npy holds the float32 image [H, W, 3], rows top-down.

With --move-object OBJ --move-by DX DY DZ the orbit also drags an object: object OBJ of the scene file is translated by the total
(DX, DY, DZ) in FRAMES equal steps through PathTracer.SetObjectTransform (a BVH refit per step, no rebuild), and with --temporal
each step ends in PathTracer.TemporalFrameMoving (include/ptk.h ptk_temporal_frame_moving) under PathTracer.TrackMotion, so that
the object's samples follow it instead of being thrown away or smeared.  --motion-vectors FILE.npy writes the last step's
screen-space motion vectors, float32 [H, W, 2] = (columns, rows) from each pixel to where its surface point was in the step before,
rows top-down, NaN where the pixel sees nothing.

With --temporal --denoise --temporal-variance each step ends in PathTracer.TemporalFrameMoments instead (include/ptk.h
ptk_temporal_frame_moments; with --move-object in its moving mode), which carries the moments of demodulated luminance beside the
colour; the last step is followed by PathTracer.TemporalVariance and PathTracer.DenoiseTemporal, so the a-trous filter weighs
luminance differences in standard deviations of each pixel's accumulated value and the chain never leaves the device.  The PNG and
--npy hold that result.

With --equirect WIDTH the image is a WIDTH x WIDTH/2 latitude-longitude panorama from the scene's camera position, traced through
PathTracer.TraceRays (include/ptk.h ptk_trace_rays; rays.equirect_rays) instead of the perspective camera.

With --equirect WIDTH --hits FILE.npz nothing is traced and no image written: the .npz holds what the panorama's rays hit
(PathTracer.IntersectRays, include/ptk.h ptk_intersect_rays, sample 0) - depth, triangle, material [H, W] and bary [H, W, 2], rows
top-down - a depth panorama; --spp is not needed.  With --attributes the .npz also holds what is at the hits
(PathTracer.SurfaceAttributes, include/ptk.h ptk_surface_attributes): normal - the shading normal, towards the camera -, albedo
and emission [H, W, 3]; the other arrays are what they are without it.  With --layers K (1 .. 16) the .npz also holds the first K surfaces along each
ray in order (PathTracer.MultiHitRays, include/ptk.h ptk_multihit_rays - geometry only, opacity maps take no part): layer_t and
layer_tri [K, H, W] (+inf and -1 behind a ray's last surface) and layer_count [H, W]; the other arrays are what they are without it.

With --point-cloud N no image is written: the .npz holds N points of the scene's surface, drawn in proportion to area
(PathTracer.SampleSurface, include/ptk.h ptk_sample_surface, sample 0 of --seed), each traced with --spp samples along the lightmap
bake's ray - from the point lifted by --offset along its face normal (default: 1e-3 of the scene extent), against the normal -
through surface.bake_points: position, normal [N, 3] float32, triangle, material [N] int32 and radiance [N, 3] float32, the sum over
the samples - and the points' albedo, shading_normal and emission [N, 3] float32 (ptk_surface_attributes).  A bake that needs
neither vertices nor a uv layout.

With --bake-lightmap SIZE the image is a SIZE x SIZE lightmap (include/ptk.h ptk_bake_lightmap): per texel of the scene's own uv
layout - or, with --bake-atlas, of lightmap.grid_atlas, one chart per triangle - the radiance leaving the surface along its normal,
baked by PathTracer.BakeLightmap and padded by --dilate K passes of ptk_lightmap_dilate.

With --bake-probes NX NY NZ the output is an .npz of irradiance probes (include/ptk.h ptk_bake_probes): a grid of NX x NY x NZ probes
that spans the scene's vertex bounds, --probe-dirs directions of probes.fibonacci_dirs each, baked by PathTracer.BakeProbes; it holds
coefs [NZ, NY, NX, 9, 3], dims, origin and spacing - the arguments of ptk_probes_irradiance / PathTracer.SampleProbes.  With
--probe-visibility RES it also holds the probes' depth moments (include/ptk.h ptk_bake_probe_visibility, sample 0, over the same
directions): moments [NZ, NY, NX, RES * RES, 2], res and max_dist (--probe-max-dist, by default probes.default_max_dist of the
spacing) - the further arguments of ptk_probes_irradiance_visible / PathTracer.SampleProbesVisible.

With --distance-field NX NY NZ the output is an .npz of the distance from each point of a grid of NX x NY x NZ points that spans the
scene's vertex bounds (probes.grid_over_bounds / grid_positions) to the nearest surface (PathTracer.closest_points, include/ptk.h
ptk_closest_points): dist [NZ, NY, NX] (inf beyond --df-max-dist), tri, point [NZ, NY, NX, 3], origin, spacing and side - the sign of
dot(p - point, face normal of tri), +1 / -1 / 0.  side is per FACE: it says which side of the nearest triangle's plane the point is
on and is not a watertight inside / outside test (open meshes, inconsistent winding and points nearest to an edge or a vertex
have no such thing).  With --signed the .npz also holds that test: inside [NZ, NY, NX] uint8 (PathTracer.contains_points,
include/ptk.h ptk_contains_points, the built-in directions; --inside-mode winding, the default, or parity) and sdf = dist with its
sign bit set where inside (ptk_signed_distance: -inf inside and beyond --df-max-dist); every other array is what it is without
--signed, byte for byte.

With --voxelize NX NY NZ the output is an .npz of a surface voxelisation over the same grid (overlap.voxel_occupancy through
PathTracer.overlap_boxes, include/ptk.h ptk_overlap_boxes): occupancy [NZ, NY, NX] bool, True where a triangle meets the closed box
that reaches half a spacing around the grid point, with origin and spacing; --solid also sets the voxels whose centre
PathTracer.contains_points finds inside the closed geometry.

The headless equivalent of the reference's Start button + Export (main.cpp:3563-3618, :760-771):
LoadScene -> SendObjectsToPathTracer -> RenderFrame() x spp -> PNG (flipped to top-down)."""
from __future__ import annotations

import argparse
import sys
import time

import numpy as np


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("-o", "--out", default="render.png")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--pinhole", action="store_true", help="SetCameraAperture(0) after loading")
    ap.add_argument("--noise-threshold", type=float, default=None,
                    help="adaptive render: relative noise target per pixel (--spp is then the maximum)")
    ap.add_argument("--min-spp", type=int, default=None, help="adaptive: samples before the first test (default: 2 x step)")
    ap.add_argument("--step", type=int, default=8, help="adaptive: samples per round (default 8)")
    ap.add_argument("--denoise", action="store_true",
                    help="filter the frame (or, with --bake-lightmap, the lightmap; with --equirect, the panorama) with the a-trous denoiser before it is written; "
                         "with --noise-threshold the frame's filter is variance-guided")
    ap.add_argument("--denoise-iterations", type=int, default=None, metavar="K", help="--denoise: a-trous iterations, 1..8 (default 5)")
    ap.add_argument("--display", choices=("linear", "reinhard", "aces"), default=None,
                    help="write the frame after the display transform - exposure, this tone curve, the sRGB transfer - instead of the "
                         "plain resolve; takes the --denoise or --temporal result where there is one; with --orbit the exposure adapts "
                         "from step to step")
    ap.add_argument("--exposure", default="auto", metavar="auto|EV",
                    help="--display: metered from the frame's luminance histogram (default), or a fixed 2^EV")
    ap.add_argument("--key", type=float, default=None, metavar="K", help="--display: the value the metered average is brought to (default 0.18)")
    ap.add_argument("--adapt", type=float, default=None, metavar="A",
                    help="--display --orbit: the step toward the metered exposure per frame (default 1: no lag)")
    ap.add_argument("--linear-transfer", action="store_true", help="--display: encode linearly instead of with the sRGB transfer")
    ap.add_argument("--upscale", type=float, default=None, metavar="S",
                    help="trace the frame at 1/S of the scene file's resolution (adjusted to the same aspect ratio) and bring it up by "
                         "guided upsampling; with --denoise the low frame is denoised first, with --display the full one is shown")
    ap.add_argument("--fill-holes", type=int, default=None, metavar="SPP",
                    help="--upscale: trace the pixels no low-resolution sample could serve with SPP samples each")
    ap.add_argument("--orbit", type=int, default=None, metavar="FRAMES",
                    help="turn the camera about the scene's centre in FRAMES steps, --spp samples after a reset at each; the image is the last view")
    ap.add_argument("--orbit-degrees", type=float, default=10.0, metavar="D", help="--orbit: the whole turn in degrees (default 10)")
    ap.add_argument("--temporal", action="store_true", help="--orbit: carry each step's samples into the next by temporal reprojection")
    ap.add_argument("--temporal-variance", action="store_true",
                    help="--orbit --temporal --denoise: carry luminance moments through the reprojection and guide the denoiser by their variance")
    ap.add_argument("--move-object", type=int, default=None, metavar="OBJ", help="--orbit: also translate object OBJ of the scene file, by --move-by over the steps")
    ap.add_argument("--move-by", type=float, nargs=3, default=None, metavar=("DX", "DY", "DZ"), help="--move-object: the whole translation in world units")
    ap.add_argument("--motion-vectors", metavar="FILE.npy", default=None,
                    help="--move-object with --temporal: write the last step's motion vectors, float32 [H, W, 2], rows top-down")
    ap.add_argument("--features", metavar="FILE.npz", default=None,
                    help="also write the first-hit feature planes (depth, triangle, material, bary, position, normal_geom, normal, "
                         "albedo, emission, gloss; sample 0) to this .npz, rows top-down like the PNG")
    ap.add_argument("--equirect", type=int, metavar="WIDTH", default=None,
                    help="render a WIDTH x WIDTH/2 latitude-longitude panorama about the scene's camera instead of its perspective view")
    ap.add_argument("--npy", metavar="FILE.npy", default=None,
                    help="--equirect: also write the float32 sums over the samples, [H, W, 3], rows top-down (mean = sum / spp)")
    ap.add_argument("--hits", metavar="FILE.npz", default=None,
                    help="--equirect: instead of tracing, write what the panorama's rays hit (depth, triangle, material, bary; rows "
                         "top-down) to this .npz")
    ap.add_argument("--layers", type=int, metavar="K", default=None,
                    help="--hits: also write the first K (1 .. 16) surfaces along each ray in order: layer_t, layer_tri [K, H, W] "
                         "and layer_count [H, W]")
    ap.add_argument("--attributes", action="store_true",
                    help="--hits: also write what is at the hits: normal (the shading normal, towards the camera), albedo and "
                         "emission [H, W, 3]")
    ap.add_argument("--bake-lightmap", type=int, metavar="SIZE", default=None,
                    help="bake a SIZE x SIZE lightmap over the scene's uvs instead of rendering a view; the PNG holds the mean "
                         "(sum / spp) resolved like a frame, rows top-down; --npy the float32 sums [SIZE, SIZE, 3], rows bottom-up as baked")
    ap.add_argument("--bake-atlas", action="store_true", help="--bake-lightmap: lay the triangles out with lightmap.grid_atlas")
    ap.add_argument("--point-cloud", type=int, metavar="N", default=None,
                    help="instead of rendering a view, sample N points of the scene's surface by area and bake each with --spp samples "
                         "along its normal; -o names the .npz (position, normal, triangle, material, radiance)")
    ap.add_argument("--offset", type=float, default=None,
                    help="--point-cloud: distance of the ray origins from the surface (default: 1e-3 of the scene extent)")
    ap.add_argument("--bake-offset", type=float, default=None,
                    help="--bake-lightmap: distance of the ray origins from the surface (default: 1e-3 of the scene extent)")
    ap.add_argument("--bake-back", action="store_true", help="--bake-lightmap: bake the back side (PTK_BAKE_BACK)")
    ap.add_argument("--dilate", type=int, default=0, metavar="K", help="--bake-lightmap: chart padding passes")
    ap.add_argument("--bake-probes", type=int, nargs=3, metavar=("NX", "NY", "NZ"), default=None,
                    help="bake a grid of NX x NY x NZ irradiance probes over the scene's vertex bounds instead of rendering a view; "
                         "-o names an .npz with coefs [NZ, NY, NX, 9, 3], dims, origin, spacing")
    ap.add_argument("--probe-dirs", type=int, default=256, metavar="D", help="--bake-probes: directions per probe (default 256)")
    ap.add_argument("--probe-visibility", type=int, default=None, metavar="RES",
                    help="--bake-probes: also bake RES x RES depth moments per probe (1..16) and add moments, res, max_dist to the .npz")
    ap.add_argument("--probe-max-dist", type=float, default=None, metavar="M",
                    help="--probe-visibility: distance the depths are clamped to (default: 1.5 x the grid's cell diagonal)")
    ap.add_argument("--distance-field", type=int, nargs=3, metavar=("NX", "NY", "NZ"), default=None,
                    help="instead of rendering a view, write the distance to the nearest surface over a grid of NX x NY x NZ points that "
                         "spans the scene's vertex bounds; -o names an .npz with dist, tri, point, origin, spacing and side.  side is the "
                         "sign of dot(p - point, face normal of tri): per face, NOT a watertight inside / outside test")
    ap.add_argument("--df-max-dist", type=float, default=None, metavar="M",
                    help="--distance-field: only surface strictly nearer than M counts (dist inf, tri -1, side 0 beyond it)")
    ap.add_argument("--signed", action="store_true",
                    help="--distance-field: add inside (uint8: the point lies inside the closed geometry) and sdf (dist, negative inside) "
                         "to the .npz")
    ap.add_argument("--inside-mode", choices=("winding", "parity"), default="winding",
                    help="--signed: a ray votes inside when it crosses unequal numbers of back and front faces (winding: any consistently "
                         "wound closed mesh) or an odd number of faces (parity: closed meshes wound inconsistently)")
    ap.add_argument("--nearest", type=int, default=None, metavar="K",
                    help="--distance-field: the K (1..16) nearest triangles per grid point (PathTracer.nearest_triangles): the .npz holds "
                         "count, and tri, dist, point with a trailing K axis (-1 / inf / 0 behind count), origin and spacing")
    ap.add_argument("--voxelize", type=int, nargs=3, metavar=("NX", "NY", "NZ"), default=None,
                    help="instead of rendering a view, write which voxels of a grid of NX x NY x NZ voxels centred on the --distance-field "
                         "grid's points hold surface; -o names an .npz with occupancy [NZ, NY, NX] bool, origin and spacing")
    ap.add_argument("--solid", action="store_true", help="--voxelize: also set the voxels whose centre lies inside the closed geometry")
    return ap


def resolve_mean(total, spp):
    """mean = sum / spp resolved to 8 bits by the frame's own rule (pathtracer.cpp:802-812: clamped to [0, 1], NaN to 0, x * 255
    truncated)"""
    with np.errstate(all="ignore"):
        x = total / np.float32(spp)
    x = np.where(x < 0, np.float32(0), np.where(x > 1, np.float32(1), x))
    x = np.where(np.isnan(x), np.float32(0), x).astype(np.float32)
    return (x * np.float32(255)).astype(np.uint8)


def adaptive_args(a):
    """(threshold, min_spp, step, max_spp) of an adaptive call: --spp is the maximum, --min-spp defaults to 2 x step"""
    return a.noise_threshold, a.min_spp if a.min_spp is not None else min(2 * a.step, a.spp), a.step, a.spp


def mean_of(total, counts):
    """sum / count in float32, 0 where the count is 0"""
    with np.errstate(all="ignore"):
        m = total / counts.astype(np.float32)[..., None]
    return np.where(counts[..., None] == 0, np.float32(0), m).astype(np.float32)


def counts_path(npy: str) -> str:
    return (npy[:-4] if npy.endswith(".npy") else npy) + ".counts.npy"


def bake_offset(pt) -> float:
    """the default --bake-offset: 1e-3 of the largest side of the staged scene's bounding box"""
    v = np.asarray(pt.StagedScene()["verts"], np.float64).reshape(-1, 3)
    return float(np.float32(1e-3 * (v.max(axis=0) - v.min(axis=0)).max())) if len(v) else 1e-3


def display_params(a):
    """ptk.display_defaults with --display, --exposure, --key, --adapt and --linear-transfer"""
    from . import ptk
    p = ptk.display_defaults(op={"linear": ptk.DISPLAY_LINEAR, "reinhard": ptk.DISPLAY_REINHARD, "aces": ptk.DISPLAY_ACES}[a.display])
    if a.exposure != "auto":
        p.mode, p.exposure = ptk.EXPOSURE_MANUAL, float(2.0 ** float(a.exposure))
    if a.key is not None:
        p.key = a.key
    if a.adapt is not None:
        p.adapt = a.adapt
    if a.linear_transfer:
        p.transfer = ptk.TRANSFER_LINEAR
    return p


def denoise_params(pt, a, variance=False):
    """ptk.denoise_defaults for the staged scene's extent, with --denoise-iterations"""
    from . import ptk
    v = np.asarray(pt.StagedScene()["verts"], np.float64).reshape(-1, 3)
    p = ptk.denoise_defaults(float(np.linalg.norm(v.max(axis=0) - v.min(axis=0))) if len(v) else 1.0, variance)
    if a.denoise_iterations is not None:
        p.iterations = a.denoise_iterations
    return p


def denoise_lightmap(pt, a, mean, owner, size, uvs):
    """--bake-lightmap --denoise: lightmap.denoise over the covered texels, guided by their positions and shading normals and
    demodulated by their albedo (lightmap.guides)"""
    from .lightmap import denoise, guides
    cover_owner, bary, pos = pt.BakeCoverage(size, size, uvs=uvs)
    albedo, normals = guides(pt, cover_owner, bary)
    if a.bake_back:
        normals = -normals
    return denoise(pt.context(), np.ascontiguousarray(mean, np.float32), owner, pos, normals, params=denoise_params(pt, a), albedo=albedo)


def render_lightmap(pt, a) -> int:
    from .lightmap import grid_atlas
    from .pathtracer import export_png
    size = a.bake_lightmap
    if size < 1 or size > 16384 or a.spp < 1 or a.dilate < 0:
        print("error: --bake-lightmap needs a size in 1..16384, --spp of at least 1 and --dilate of at least 0", file=sys.stderr)
        return 1
    uvs = grid_atlas(pt.GetTriangleCount(), size, size) if a.bake_atlas else None
    offset = a.bake_offset if a.bake_offset is not None else bake_offset(pt)
    t1 = time.time()
    if a.noise_threshold is not None:
        return render_lightmap_adaptive(pt, a, size, uvs, offset)
    total, owner = pt.BakeLightmap(size, size, offset, 0, a.spp, uvs=uvs, back=a.bake_back)
    covered = int((owner >= 0).sum())
    if a.denoise:
        # (the mean scaled back by spp: --npy keeps holding sums, and the padding below copies denoised texels)
        total = denoise_lightmap(pt, a, total / np.float32(a.spp), owner, size, uvs) * np.float32(a.spp)
    if a.dilate:
        pt.DilateLightmap(total, owner, a.dilate)
    t2 = time.time()
    export_png(a.out, resolve_mean(total, a.spp))       # (the bake's rows are bottom-up, as export_png takes them: top-down in the file)
    if a.npy:
        np.save(a.npy, total)
    print(f"{a.scene}: {pt.GetTriangleCount()} triangles, {size}x{size} lightmap, {covered} texels covered, {a.spp} spp, "
          f"depth {pt.GetTraceDepth()}, offset {offset:g}: {t2 - t1:.3f} s ({covered * a.spp / (t2 - t1) / 1e6:.0f} Msamples/s) -> {a.out}")
    return 0


def render_lightmap_adaptive(pt, a, size, uvs, offset) -> int:
    """--bake-lightmap with --noise-threshold: the mean per texel, padded like a plain bake"""
    from .pathtracer import export_png
    t1 = time.time()
    total, counts, owner, res = pt.BakeLightmapAdaptive(size, size, offset, *adaptive_args(a), uvs=uvs, back=a.bake_back)
    covered = int((owner >= 0).sum())
    mean = mean_of(total, counts)
    if a.denoise:
        mean = denoise_lightmap(pt, a, mean, owner, size, uvs)
    if a.dilate:
        pt.DilateLightmap(mean, owner, a.dilate)
    t2 = time.time()
    export_png(a.out, resolve_mean(mean, 1))
    if a.npy:
        np.save(a.npy, mean)
        np.save(counts_path(a.npy), counts)
    print(f"{a.scene}: {pt.GetTriangleCount()} triangles, {size}x{size} lightmap, {covered} texels covered, depth {pt.GetTraceDepth()}, "
          f"offset {offset:g}: {t2 - t1:.3f} s -> {a.out}")
    print(f"adaptive (threshold {a.noise_threshold}): {res['ray_samples']} texel samples of {covered * a.spp} "
          f"({res['ray_samples'] / max(covered * a.spp, 1):.3f}), {res['rounds']} rounds, {res['active_rays']} texels still active")
    return 0


def render_probes(pt, a) -> int:
    from .probes import default_max_dist, fibonacci_dirs, grid_over_bounds, grid_positions, sh_weight
    dims = tuple(a.bake_probes)
    if min(dims) < 1 or not 1 <= a.probe_dirs <= 65536 or a.spp < 1:
        print("error: --bake-probes needs dims of at least 1, --probe-dirs in 1..65536 and --spp of at least 1", file=sys.stderr)
        return 1
    if a.probe_visibility is not None and not 1 <= a.probe_visibility <= 16:
        print("error: --probe-visibility needs a resolution in 1..16", file=sys.stderr)
        return 1
    if a.probe_max_dist is not None and (a.probe_visibility is None or not 0.0 < a.probe_max_dist <= 1e18):
        print("error: --probe-max-dist goes with --probe-visibility and needs a distance > 0 and at most 1e18", file=sys.stderr)
        return 1
    v = np.asarray(pt.StagedScene()["verts"], np.float64).reshape(-1, 3)
    if not len(v):
        print("error: --bake-probes: the scene has no triangles", file=sys.stderr)
        return 1
    origin, spacing = grid_over_bounds(v.min(axis=0), v.max(axis=0), dims)
    pos = grid_positions(dims, origin, spacing)
    t1 = time.time()
    dirs = fibonacci_dirs(a.probe_dirs)
    _, coefs = pt.BakeProbes(pos, dirs, 0, a.spp, sh_weight(a.probe_dirs, a.spp))
    t2 = time.time()
    fields = dict(coefs=coefs.reshape(dims[2], dims[1], dims[0], 9, 3), dims=np.array(dims, np.int32), origin=origin, spacing=spacing)
    if a.probe_visibility is not None:
        res = a.probe_visibility
        max_dist = a.probe_max_dist if a.probe_max_dist is not None else default_max_dist(spacing)
        _, moments = pt.BakeProbeVisibility(pos, dirs, res, max_dist)
        fields.update(moments=moments.reshape(dims[2], dims[1], dims[0], res * res, 2), res=np.int32(res), max_dist=np.float32(max_dist))
    t3 = time.time()
    with open(a.out, "wb") as f:                # (np.savez would append .npz to another suffix)
        np.savez(f, **fields)
    rays = len(pos) * a.probe_dirs
    print(f"{a.scene}: {pt.GetTriangleCount()} triangles, {dims[0]}x{dims[1]}x{dims[2]} probes x {a.probe_dirs} directions, {a.spp} spp, "
          f"depth {pt.GetTraceDepth()}: {t2 - t1:.3f} s ({rays * a.spp / (t2 - t1) / 1e6:.0f} Msamples/s) -> {a.out}")
    if a.probe_visibility is not None:
        print(f"visibility: {a.probe_visibility}x{a.probe_visibility} depth moments per probe, max_dist {max_dist:g}: {t3 - t2:.3f} s "
              f"({rays / (t3 - t2) / 1e6:.0f} Mrays/s)")
    return 0


def face_side(verts, points, point, tri):
    """the sign (+1, -1, 0; int8) of dot(p - point, cross(v2 - v1, v3 - v1) of triangle tri), in float32; 0 on a miss"""
    t = np.asarray(verts, np.float32).reshape(-1, 3, 3)[np.maximum(tri, 0)]
    with np.errstate(all="ignore"):
        nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]).astype(np.float32)
        s = np.sign(((points - point) * nrm).sum(axis=1, dtype=np.float32))
    return np.where((tri >= 0) & np.isfinite(s), s, 0).astype(np.int8)


def render_distance_field(pt, a) -> int:
    from .probes import grid_over_bounds, grid_positions
    dims = tuple(a.distance_field)
    if min(dims) < 1 or (a.df_max_dist is not None and not a.df_max_dist > 0.0):
        print("error: --distance-field needs dims of at least 1 and --df-max-dist a distance > 0", file=sys.stderr)
        return 1
    verts = np.asarray(pt.StagedScene()["verts"], np.float32).reshape(-1, 9)
    if not len(verts):
        print("error: --distance-field: the scene has no triangles", file=sys.stderr)
        return 1
    v = verts.reshape(-1, 3).astype(np.float64)
    origin, spacing = grid_over_bounds(v.min(axis=0), v.max(axis=0), dims)
    pos = grid_positions(dims, origin, spacing)
    t1 = time.time()
    md = None if a.df_max_dist is None else np.full(len(pos), a.df_max_dist, np.float32)
    extra = {}
    shape = (dims[2], dims[1], dims[0])
    if a.nearest is not None:                   # the K nearest triangles per grid point: a trailing K axis
        K = a.nearest
        count, tri, dist, point, _ = pt.nearest_triangles(pos, K, md)
        t2 = time.time()
        with open(a.out, "wb") as f:
            np.savez(f, count=count.reshape(shape), dist=dist.reshape(shape + (K,)), tri=tri.reshape(shape + (K,)),
                     point=point.reshape(shape + (K, 3)), origin=origin, spacing=spacing)
        print(f"{a.scene}: {pt.GetTriangleCount()} triangles, {dims[0]}x{dims[1]}x{dims[2]} distance field of the {K} nearest, "
              f"{int((count > 0).sum())} points within reach: {t2 - t1:.3f} s -> {a.out}")
        return 0
    if a.signed:
        tri, sdf, point, _ = pt.signed_distance(pos, md, None, a.inside_mode)
        dist = np.abs(sdf)                      # (clears the sign bit: ptk_closest_points' dist, bit for bit)
        extra = dict(inside=np.signbit(sdf).astype(np.uint8).reshape(shape), sdf=sdf.reshape(shape))
    else:
        tri, dist, point, _ = pt.closest_points(pos, md)
    t2 = time.time()
    with open(a.out, "wb") as f:                # (np.savez would append .npz to another suffix)
        np.savez(f, dist=dist.reshape(shape), tri=tri.reshape(shape), point=point.reshape(shape + (3,)), origin=origin, spacing=spacing,
                 side=face_side(verts, pos, point, tri).reshape(shape), **extra)
    print(f"{a.scene}: {pt.GetTriangleCount()} triangles, {dims[0]}x{dims[1]}x{dims[2]} distance field, "
          f"{int((tri >= 0).sum())} points within reach: {t2 - t1:.3f} s -> {a.out}")
    return 0


def render_voxels(pt, a) -> int:
    from .overlap import voxel_occupancy
    from .probes import grid_over_bounds
    dims = tuple(a.voxelize)
    if min(dims) < 1:
        print("error: --voxelize needs dims of at least 1", file=sys.stderr)
        return 1
    v = np.asarray(pt.StagedScene()["verts"], np.float64).reshape(-1, 3)
    if not len(v):
        print("error: --voxelize: the scene has no triangles", file=sys.stderr)
        return 1
    origin, spacing = grid_over_bounds(v.min(axis=0), v.max(axis=0), dims)
    t1 = time.time()
    occ = voxel_occupancy(pt, origin, spacing, dims, solid=a.solid)
    t2 = time.time()
    with open(a.out, "wb") as f:                # (np.savez would append .npz to another suffix)
        np.savez(f, occupancy=occ, origin=origin, spacing=spacing)
    print(f"{a.scene}: {pt.GetTriangleCount()} triangles, {dims[0]}x{dims[1]}x{dims[2]} voxels, {int(occ.sum())} occupied: "
          f"{t2 - t1:.3f} s -> {a.out}")
    return 0


class _TracerSurface:
    """surface.bake_points' and rays.hit_guides' view of a PathTracer: sample_surface, trace_rays, intersect_rays and
    surface_attributes at the tracer's own seed and trace depth"""

    def __init__(self, pt):
        self.pt = pt

    def sample_surface(self, n, seed=0, key_base=0, sample=0):
        return self.pt.SampleSurface(n, key_base=key_base, sample=sample)

    def trace_rays(self, origins, dirs, max_depth, first_sample, spp, seed, key_base=0, out=None):
        return self.pt.TraceRays(origins, dirs, first_sample, spp, key_base=key_base, out=out)

    def intersect_rays(self, origins, dirs, sample=0, seed=0, key_base=0):
        return self.pt.IntersectRays(origins, dirs, sample, key_base=key_base)

    def surface_attributes(self, tri, bary, dirs=None, want=None):
        return self.pt.SurfaceAttributes(tri, bary, dirs) if want is None else self.pt.SurfaceAttributes(tri, bary, dirs, want)


def render_point_cloud(pt, a) -> int:
    """--point-cloud: surface.bake_points over the whole surface, written as arrays"""
    from . import surface
    if a.point_cloud < 1 or a.spp < 1 or (a.offset is not None and not a.offset >= 0.0):
        print("error: --point-cloud needs N >= 1, --spp >= 1 and --offset >= 0", file=sys.stderr)
        return 1
    if not pt.GetTriangleCount():
        print("error: --point-cloud: the scene has no triangles", file=sys.stderr)
        return 1
    offset = a.offset if a.offset is not None else bake_offset(pt)
    t1 = time.time()
    position, normal, tri, material, radiance, at = surface.bake_points(_TracerSurface(pt), a.point_cloud, a.spp, offset, pt.GetTraceDepth(),
                                                                        seed=a.seed, attributes=True)
    t2 = time.time()
    with open(a.out, "wb") as f:                # (np.savez would append .npz to another suffix)
        np.savez(f, position=position, normal=normal, triangle=tri, material=material, radiance=radiance, spp=np.int32(a.spp),
                 offset=np.float32(offset), albedo=at["albedo"], shading_normal=at["normal"], emission=at["emission"])
    print(f"{a.scene}: {pt.GetTriangleCount()} triangles, {a.point_cloud} surface points, {a.spp} spp, depth {pt.GetTraceDepth()}: "
          f"{t2 - t1:.3f} s -> {a.out}")
    return 0


def render_equirect(pt, a) -> int:
    """The panorama: one TraceRays call over the pixel centres' rays, mean = sum / spp resolved to 8 bits by the frame's own rule
    (pathtracer.cpp:802-812: clamped to [0, 1], NaN to 0, x * 255 truncated)."""
    from . import ptk
    from .pathtracer import export_png
    from .rays import equirect_rays, hit_guides
    w, h = a.equirect, a.equirect // 2
    if h < 1 or a.spp < 1:
        print("error: --equirect needs a width of at least 2 and --spp of at least 1", file=sys.stderr)
        return 1
    origins, dirs = equirect_rays(*pt.GetCamera(), w, h)
    t1 = time.time()
    if a.hits:
        tri, t, bary, material = pt.IntersectRays(origins, dirs)
        planes = dict(depth=t.reshape(h, w), triangle=tri.reshape(h, w), material=material.reshape(h, w), bary=bary.reshape(h, w, 2))
        if a.attributes:
            at = pt.SurfaceAttributes(tri, bary, dirs, 1 << ptk.ATTR_NORMAL | 1 << ptk.ATTR_ALBEDO | 1 << ptk.ATTR_EMISSION)
            planes.update(normal=at["normal"].reshape(h, w, 3), albedo=at["albedo"].reshape(h, w, 3), emission=at["emission"].reshape(h, w, 3))
        if a.layers is not None:
            count, ltri, lt, _, _ = pt.MultiHitRays(origins, dirs, a.layers)
            planes.update(layer_t=np.ascontiguousarray(lt.T).reshape(a.layers, h, w),
                          layer_tri=np.ascontiguousarray(ltri.T).reshape(a.layers, h, w), layer_count=count.reshape(h, w))
        t2 = time.time()
        with open(a.hits, "wb") as f:               # (np.savez would append .npz to another suffix)
            np.savez(f, **planes)
        print(f"{a.scene}: {pt.GetTriangleCount()} triangles, {w}x{h} panorama, {int((tri >= 0).sum())} of {w * h} rays hit: "
              f"{t2 - t1:.3f} s -> {a.hits}")
        return 0
    if a.noise_threshold is not None:
        total, _, counts, res = pt.TraceRaysAdaptive(origins, dirs, *adaptive_args(a))
        mean = mean_of(total.reshape(h, w, 3), counts.reshape(h, w))
        t2 = time.time()
        export_png(a.out, resolve_mean(mean, 1)[::-1].copy())
        if a.npy:
            np.save(a.npy, mean)
            np.save(counts_path(a.npy), counts.reshape(h, w))
        print(f"{a.scene}: {pt.GetTriangleCount()} triangles, {w}x{h} panorama, depth {pt.GetTraceDepth()}: {t2 - t1:.3f} s -> {a.out}")
        print(f"adaptive (threshold {a.noise_threshold}): {res['ray_samples']} ray samples of {w * h * a.spp} "
              f"({res['ray_samples'] / (w * h * a.spp):.3f}), {res['rounds']} rounds, {res['active_rays']} rays still active")
        return 0
    total = pt.TraceRays(origins, dirs, 0, a.spp).reshape(h, w, 3)
    if a.denoise:
        # the sums over the samples through the a-trous filter, guided by what the panorama's rays hit (rays.hit_guides)
        g = hit_guides(_TracerSurface(pt), origins, dirs)
        total = pt.context().denoise_planes(np.ascontiguousarray(total), g["id"].reshape(h, w), g["normal"].reshape(h, w, 3),
                                            g["position"].reshape(h, w, 3), denoise_params(pt, a), albedo=g["albedo"].reshape(h, w, 3))
    t2 = time.time()
    with np.errstate(all="ignore"):
        x = total / np.float32(a.spp)
    x = np.where(x < 0, np.float32(0), np.where(x > 1, np.float32(1), x))
    x = np.where(np.isnan(x), np.float32(0), x).astype(np.float32)
    export_png(a.out, (x * np.float32(255)).astype(np.uint8)[::-1].copy())
    if a.npy:
        np.save(a.npy, total)
    print(f"{a.scene}: {pt.GetTriangleCount()} triangles, {w}x{h} panorama, {a.spp} spp, depth {pt.GetTraceDepth()}: "
          f"{t2 - t1:.3f} s ({w * h * a.spp / (t2 - t1) / 1e6:.0f} Msamples/s) -> {a.out}")
    return 0


class _TracerRays:
    """upscale.fill_holes' view of a PathTracer: trace_rays at the tracer's own seed and trace depth"""

    def __init__(self, pt):
        self.pt = pt

    def trace_rays(self, origins, dirs, max_depth, first_sample, spp, seed, key_base=0):
        return self.pt.TraceRays(origins, dirs, first_sample, spp, key_base=key_base)


def render_upscaled(pt, a, export_png) -> int:
    """--upscale: the frame traced at a low resolution, (denoised,) upsampled to the scene file's, (its holes traced,) (displayed)"""
    from . import ptk, upscale
    W, H = pt.GetResolution()
    w, h = upscale.low_resolution(W, H, a.upscale)
    pt.SetResolution((w, h))
    low = np.zeros((h, w, 3), np.uint8)
    pt.SetOutImage(low)
    t1 = time.time()
    pt.RenderFrames(a.spp)
    if pt.LastError():
        raise RuntimeError(pt.LastError())
    if a.denoise:
        pt.DenoiseFrame(denoise_params(pt, a))
    pt.RenderGuides(W, H)
    pt.UpsampleFrame(ptk.UPSAMPLE_DENOISED if a.denoise else ptk.UPSAMPLE_ACCUM)
    color, cls = pt.ReadUpsampled()
    t2 = time.time()
    valid = pt.ReadGuide(ptk.FEAT_MATERIAL) >= 0
    shares = upscale.class_shares(cls, valid)
    filled = 0
    if a.fill_holes:
        color, info = upscale.fill_holes(_TracerRays(pt), color, cls, pt.context().guide_view(), a.fill_holes, pt.GetTraceDepth(), key_base=w * h)
        filled = len(info["rows"])
    if a.display:
        out = pt.context().display_planes(color, display_params(a))
    else:
        out = resolve_mean(color, 1)
    export_png(a.out, out)
    if a.npy:
        np.save(a.npy, color[::-1].copy())
    print(f"{a.scene}: {pt.GetTriangleCount()} triangles, traced {w}x{h} at {a.spp} spp, shown {W}x{H} (x{W / w:.3g}): "
          f"render + upsample {t2 - t1:.3f} s -> {a.out}")
    print(f"upsample classes over the {int(valid.sum())} pixels that see the scene: bilinear {shares[0]:.4f}, wide ring {shares[1]:.4f}, "
          f"holes {shares[2]:.4f}" + (f"; {filled} holes traced at {a.fill_holes} spp" if a.fill_holes else ""))
    return 0


def orbit_cameras(pt, frames: int, degrees: float):
    """(pos, dir, up) of the loaded camera turned about the vertical axis through the centre of the staged scene's bounds, after each
    of `frames` equal steps of degrees / frames"""
    v = np.asarray(pt.StagedScene()["verts"], np.float64).reshape(-1, 3)
    centre = (v.max(axis=0) + v.min(axis=0)) / 2 if len(v) else np.zeros(3)
    pos, dir_, up = (np.asarray(x, np.float64) for x in pt.GetCamera())
    out = []
    for k in range(1, frames + 1):
        a = np.radians(degrees * k / frames)
        R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
        out.append(tuple((x).astype(np.float32) for x in (centre + R @ (pos - centre), R @ dir_, R @ up)))
    return out


def render_orbit(pt, a) -> int:
    """--orbit: a camera drag of FRAMES steps, each a reset and --spp samples, with or without temporal reprojection"""
    from . import ptk
    from .pathtracer import export_png
    w, h = pt.GetResolution()
    out = np.zeros((h, w, 3), np.uint8)
    pt.SetOutImage(out)
    moving = a.move_object is not None
    if moving:
        base = pt.GetObjectTransform(a.move_object)
        pt.TrackMotion(True)
    t1 = time.time()
    for k, (pos, dir_, up) in enumerate(orbit_cameras(pt, a.orbit, a.orbit_degrees)):
        pt.SetCamera(pos, dir_, up)
        if moving:
            M = base.copy()
            M[3][:3] += np.asarray(a.move_by, np.float32) * np.float32((k + 1) / a.orbit)
            pt.SetObjectTransform(a.move_object, M)
        pt.ResetImage()
        pt.RenderFrames(a.spp)
        if pt.LastError():
            raise RuntimeError(pt.LastError())
        if a.temporal_variance:
            pt.TemporalFrameMoments(moving=moving)
        elif a.temporal:
            pt.TemporalFrameMoving() if moving else pt.TemporalFrame()
        if a.display and k + 1 < a.orbit:
            # the exposure state lives on the device and adapts step by step; the last step is displayed below, behind its filter
            pt.DisplayFrame(ptk.DISPLAY_TEMPORAL if a.temporal else ptk.DISPLAY_ACCUM, display_params(a))
    t2 = time.time()
    if a.motion_vectors:
        np.save(a.motion_vectors, np.ascontiguousarray(pt.ReadMotion()[2][::-1], np.float32))
    if a.temporal:
        image, count = pt.ReadTemporal()
        if a.temporal_variance:
            pt.TemporalVariance()
            pt.DenoiseTemporal(denoise_params(pt, a, True))
            image = pt.ReadDenoised()
        elif a.denoise:
            tri = pt.ReadFeature(ptk.FEAT_TRIANGLE)
            mask = np.where((pt.ReadFeature(ptk.FEAT_EMISSION) != 0).any(axis=-1), -1, tri).astype(np.int32)
            image = pt.context().denoise_planes(image, mask, pt.ReadFeature(ptk.FEAT_NORMAL), pt.ReadFeature(ptk.FEAT_POSITION),
                                                denoise_params(pt, a), albedo=pt.ReadFeature(ptk.FEAT_ALBEDO))
        found = count > np.float32(a.spp)
        note = f", {float(found.mean()):.3f} of the pixels found history, {float(count[found].mean()) if found.any() else 0.0:.1f} samples behind each"
    elif a.denoise:
        pt.DenoiseFrame(denoise_params(pt, a))
        image, note = pt.ReadDenoised(), ""
    else:
        image, note = pt.ReadAccumulation() / np.float32(a.spp), ""
    if a.display:
        if a.temporal and a.denoise and not a.temporal_variance:
            shown = pt.context().display_planes(image, display_params(a))          # (filtered on the host side just above)
        else:
            pt.DisplayFrame(ptk.DISPLAY_DENOISED if a.denoise else ptk.DISPLAY_TEMPORAL if a.temporal else ptk.DISPLAY_ACCUM, display_params(a))
            shown = pt.ReadDisplay()
        st = pt.DisplayState()
        if a.exposure == "auto":
            note += f"; exposure {float(st['exposure']):.4g} (target {float(st['target']):.4g}, metered average {float(st['lavg']):.4g})"
    else:
        shown = resolve_mean(image, 1)
    export_png(a.out, shown[::-1].copy())
    if a.npy:
        np.save(a.npy, np.ascontiguousarray(image[::-1], np.float32))
    print(f"{a.scene}: {w}x{h}, orbit of {a.orbit} steps over {a.orbit_degrees} degrees, {a.spp} spp each"
          f"{' with temporal reprojection' if a.temporal else ''}{note}: {t2 - t1:.3f} s -> {a.out}")
    return 0


def main(argv=None):
    a = build_parser().parse_args(argv)
    from .pathtracer import PathTracer, export_png
    pt = PathTracer(a.device)
    t0 = time.time()
    pt.LoadSceneFile(a.scene)
    if a.pinhole:
        pt.SetCameraAperture(0.0)
    pt.SetSeed(a.seed)
    if a.denoise_iterations is not None and not (a.denoise and 1 <= a.denoise_iterations <= 8):
        print("error: --denoise-iterations goes with --denoise and needs a count in 1..8", file=sys.stderr)
        return 1
    if a.denoise and (a.bake_probes is not None or a.distance_field is not None):
        print("error: --denoise filters a perspective frame, an --equirect panorama or a --bake-lightmap", file=sys.stderr)
        return 1
    if a.bake_probes is None and (a.probe_visibility is not None or a.probe_max_dist is not None):
        print("error: --probe-visibility and --probe-max-dist go with --bake-probes", file=sys.stderr)
        return 1
    if a.layers is not None and not (a.equirect is not None and a.hits and 1 <= a.layers <= 16):
        print("error: --layers goes with --equirect --hits and needs a count in 1..16", file=sys.stderr)
        return 1
    if a.attributes and not (a.equirect is not None and a.hits):
        print("error: --attributes goes with --equirect --hits", file=sys.stderr)
        return 1
    if a.temporal and a.orbit is None:
        print("error: --temporal goes with --orbit", file=sys.stderr)
        return 1
    if (a.move_object is None) != (a.move_by is None) or (a.move_object is not None and a.orbit is None):
        print("error: --move-object and --move-by go together and with --orbit", file=sys.stderr)
        return 1
    if a.motion_vectors and not (a.temporal and a.move_object is not None):
        print("error: --motion-vectors goes with --temporal and --move-object", file=sys.stderr)
        return 1
    if a.temporal_variance and not (a.temporal and a.denoise):
        print("error: --temporal-variance goes with --temporal and --denoise", file=sys.stderr)
        return 1
    if a.display is None and (a.exposure != "auto" or a.key is not None or a.adapt is not None or a.linear_transfer):
        print("error: --exposure, --key, --adapt and --linear-transfer go with --display", file=sys.stderr)
        return 1
    if a.display is not None:
        if a.bake_lightmap is not None or a.bake_probes is not None or a.distance_field is not None or a.equirect is not None:
            print("error: --display shows a perspective frame or an --orbit", file=sys.stderr)
            return 1
        try:
            if a.exposure != "auto":
                float(a.exposure)
            from . import ptk
            if ptk.display_check_params(display_params(a)) != ptk.PTK_OK:
                raise ValueError
        except (ValueError, OverflowError):
            print("error: --exposure takes auto or a number of stops, --key a positive number, --adapt a number >= 0", file=sys.stderr)
            return 1
    if a.fill_holes is not None and (a.upscale is None or a.fill_holes < 1):
        print("error: --fill-holes goes with --upscale and needs SPP >= 1", file=sys.stderr)
        return 1
    if a.offset is not None and a.point_cloud is None:
        print("error: --offset goes with --point-cloud", file=sys.stderr)
        return 1
    if a.point_cloud is not None and (a.upscale is not None or a.orbit is not None or a.display is not None or a.features):
        print("error: --point-cloud is a mode of its own", file=sys.stderr)
        return 1
    if a.upscale is not None:
        if a.orbit is not None or a.noise_threshold is not None or a.bake_lightmap is not None or a.bake_probes is not None or \
                a.distance_field is not None or a.equirect is not None or a.features:
            print("error: --upscale renders one plain perspective frame", file=sys.stderr)
            return 1
        try:
            return render_upscaled(pt, a, export_png)
        except (RuntimeError, ValueError) as e:
            print("error:", e, file=sys.stderr)
            return 1
    if a.orbit is not None:
        if a.orbit < 1 or a.noise_threshold is not None or a.bake_lightmap is not None or a.bake_probes is not None or \
                a.distance_field is not None or a.equirect is not None:
            print("error: --orbit needs FRAMES >= 1 and renders plain perspective frames", file=sys.stderr)
            return 1
        try:
            return render_orbit(pt, a)
        except RuntimeError as e:
            print("error:", e, file=sys.stderr)
            return 1
    if a.bake_lightmap is not None:
        try:
            return render_lightmap(pt, a)
        except (RuntimeError, ValueError) as e:
            print("error:", e, file=sys.stderr)
            return 1
    if a.bake_probes is not None:
        try:
            return render_probes(pt, a)
        except (RuntimeError, ValueError) as e:
            print("error:", e, file=sys.stderr)
            return 1
    if a.point_cloud is not None:
        if a.bake_lightmap is not None or a.bake_probes is not None or a.distance_field is not None or a.equirect is not None or \
                a.noise_threshold is not None or a.denoise:
            print("error: --point-cloud is a mode of its own", file=sys.stderr)
            return 1
        try:
            return render_point_cloud(pt, a)
        except (RuntimeError, ValueError) as e:
            print("error:", e, file=sys.stderr)
            return 1
    if a.solid and a.voxelize is None:
        print("error: --solid goes with --voxelize", file=sys.stderr)
        return 1
    if a.voxelize is not None:
        if a.bake_lightmap is not None or a.bake_probes is not None or a.distance_field is not None or a.equirect is not None or \
                a.noise_threshold is not None or a.denoise:
            print("error: --voxelize is a mode of its own", file=sys.stderr)
            return 1
        try:
            return render_voxels(pt, a)
        except (RuntimeError, ValueError) as e:
            print("error:", e, file=sys.stderr)
            return 1
    if a.nearest is not None and (a.distance_field is None or a.signed or not 1 <= a.nearest <= 16):
        print("error: --nearest K (1..16) goes with --distance-field, without --signed", file=sys.stderr)
        return 1
    if a.distance_field is not None:
        try:
            return render_distance_field(pt, a)
        except (RuntimeError, ValueError) as e:
            print("error:", e, file=sys.stderr)
            return 1
    if a.equirect is not None:
        try:
            return render_equirect(pt, a)
        except RuntimeError as e:
            print("error:", e, file=sys.stderr)
            return 1
    w, h = pt.GetResolution()
    out = np.zeros((h, w, 3), np.uint8)
    pt.SetOutImage(out)
    t1 = time.time()
    res = None
    if a.noise_threshold is None:
        pt.RenderFrames(a.spp)
    else:
        min_spp = a.min_spp if a.min_spp is not None else min(2 * a.step, a.spp)
        try:
            res = pt.RenderAdaptive(a.noise_threshold, min_spp, a.step, a.spp)
        except RuntimeError as e:
            print("error:", e, file=sys.stderr)
            return 1
    t2 = time.time()
    if pt.LastError():
        print("error:", pt.LastError(), file=sys.stderr)
        return 1
    if a.denoise:
        try:
            pt.DenoiseFrame(denoise_params(pt, a, res is not None), variance=res is not None)
            out = pt.ResolveDenoised()
            if a.npy:
                np.save(a.npy, pt.ReadDenoised()[::-1].copy())
        except RuntimeError as e:
            print("error:", e, file=sys.stderr)
            return 1
    if a.display:
        from . import ptk
        try:
            pt.DisplayFrame(ptk.DISPLAY_DENOISED if a.denoise else ptk.DISPLAY_ACCUM, display_params(a))
            out = pt.ReadDisplay()
        except RuntimeError as e:
            print("error:", e, file=sys.stderr)
            return 1
    export_png(a.out, out)
    if a.features:
        from . import ptk
        pt.RenderFeatures(ptk.FEAT_ALL)
        np.savez(a.features, **{name: pt.ReadFeature(k)[::-1].copy() for k, name in enumerate(ptk.FEAT_NAMES)})
    done = res["pixel_samples"] if res is not None else w * h * a.spp
    print(f"{a.scene}: {pt.GetTriangleCount()} triangles, {w}x{h}, {a.spp} spp: load {t1 - t0:.2f} s, "
          f"render {t2 - t1:.3f} s ({done / (t2 - t1) / 1e6:.0f} Msamples/s) -> {a.out}")
    if res is not None:
        print(f"adaptive (threshold {a.noise_threshold}): {res['pixel_samples']} pixel samples of {w * h * a.spp} "
              f"({res['pixel_samples'] / (w * h * a.spp):.3f}), {res['rounds']} rounds, "
              f"{res['active_pixels']} pixels still active")
    return 0


if __name__ == "__main__":
    sys.exit(main())
