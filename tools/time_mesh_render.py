"""Times the mesh renderer (slice3d_amd/mesh_render.py, csrc/mesh_render.hip) with device events on the stream, beside the
float64 numpy restatement of tests/render_ref.py on the host.

Workload: the marching-cubes meshes of tools/time_mesh_sdf.py (torus + sphere field at 129^3 and 257^3), normalised, one
view at 256 x 256 pixels with 4 x 4 samples per pixel (the dataset program's defaults), camera az 0.7, el 0.3, distance
1.2, scale 0.9.  Per mesh: build + fill (transforms, slab bounds, tile lists), the render kernel, the resolve pass, the
ray-face tests per sample (the kernel's counter), and the host reference on a 32 x 32 pixel image at one sample per
pixel (its own sample count is stated beside it; it is not scaled to the device's).

The three device figures come from three timed calls (3 warm-ups, median of --reps): everything, everything without the
resolve pass, and build + fill alone through the library's entry points.  render = (all without resolve) - (build +
fill); resolve = all - (all without resolve).

    python tools/time_mesh_render.py [--sizes 129 257] [--img_size 256] [--samples 4] [--reps 10] [--out profiles/mesh_render_timing.md]

Prints a markdown report (and writes it to --out).
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_mesh_sdf import device_ms, mc_mesh  # noqa: E402

CAM = dict(az=0.7, el=0.3, distance=1.2, scale=0.9)


def build_fill(r, size, samples, tile):
    """build + fill alone, through the C ABI (what SliceRenderer.render does before it launches the render kernel)"""
    from slice3d_amd.mesh_render import camera_frame, slab_frame
    L, lib = r._L, r._lib
    R, t = camera_frame(CAM["az"], CAM["el"], CAM["distance"])
    cam = np.concatenate([R.reshape(-1), [CAM["distance"], CAM["scale"]], t, slab_frame(R).reshape(-1)])
    cam_c = (C.c_double * 26)(*cam.tolist())
    nb = lib.s3d_mesh_render_workspace_bytes(r.n_vertices, r.n_faces, size, samples, tile)
    ws = torch.empty(nb, dtype=torch.uint8, device=r.device)
    st = L.stream_ptr(r.device)
    n = C.c_long(0)
    L.check(lib.s3d_mesh_render_build(r._v.data_ptr(), r.n_vertices, r._f.data_ptr(), r.n_faces, cam_c, size, samples, tile,
                                      ws.data_ptr(), nb, C.byref(n), st), "build")
    ent = torch.empty(max(n.value, 1), dtype=torch.int32, device=r.device)
    L.check(lib.s3d_mesh_render_fill(r.n_vertices, r.n_faces, size, samples, tile, ws.data_ptr(), nb, ent.data_ptr(), n.value,
                                     st), "fill")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[129, 257])
    ap.add_argument("--img_size", type=int, default=256)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host_size", type=int, default=32)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import render_ref
    from slice3d_amd.mesh_render import SliceRenderer, default_tile
    from slice3d_amd.mesh_sdf import normalize_mesh

    size, S = args.img_size, args.samples
    tile = default_tile(S)
    n_samples = (size * S) ** 2
    lines = ["# Mesh renderer: timing (`python tools/time_mesh_render.py`)", "",
             "%s, one view of %d x %d pixels at %d x %d samples per pixel (%d samples, 13 images), tiles of %d pixels, device "
             "events on the stream, 3 warm-ups, median of %d.  render = (build + fill + render) - (build + fill); resolve = "
             "(everything) - (everything without resolve)."
             % (torch.cuda.get_device_name(0), size, size, S, S, n_samples, tile, args.reps),
             "Host column: the float64 numpy restatement (`tests/render_ref.py`, vectorised over faces) on a %d x %d image at "
             "one sample per pixel (%d samples), one process on a host that shows %d cores."
             % (args.host_size, args.host_size, args.host_size ** 2, os.cpu_count()),
             "", "| grid | faces | build + fill | render | resolve | entries | tests / sample | tests / s | host reference "
             "(%d samples) |" % args.host_size ** 2, "|---|---|---|---|---|---|---|---|---|"]

    def emit():
        text = "\n".join(lines) + "\n"
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(text)
        return text

    for n in args.sizes:
        v, f = mc_mesh(n)
        vn = normalize_mesh(v.cpu().numpy())
        fn = f.cpu().numpy()
        r = SliceRenderer((torch.from_numpy(vn).cuda(), f))
        kw = dict(size=size, samples=S, **{k: CAM[k] for k in ("scale",)})
        t_all = device_ms(lambda: r.render(CAM["az"], CAM["el"], CAM["distance"], **kw), args.reps)
        t_nores = device_ms(lambda: r.render(CAM["az"], CAM["el"], CAM["distance"], resolve=False, **kw), args.reps)
        t_build = device_ms(lambda: build_fill(r, size, S, tile), args.reps)
        tests, entries = int(r.n_tests), r.n_entries
        t_render = t_nores - t_build
        t0 = time.perf_counter()
        ref = render_ref.render(vn, fn, CAM["az"], CAM["el"], CAM["distance"], CAM["scale"], size=args.host_size, S=1, chunk=8)
        t_host = (time.perf_counter() - t0) * 1e3
        got = r.render(CAM["az"], CAM["el"], CAM["distance"], scale=CAM["scale"], size=args.host_size, samples=1,
                       return_samples=True)
        same = bool((got[2].cpu().numpy() == ref["face"]).all())
        lines.append("| %d^3 | %d | %.2f ms | %.2f ms | %.2f ms | %d | %.1f | %.2e | %.0f ms (faces %s the device's) |"
                     % (n, len(fn), t_build, t_render, t_all - t_nores, entries, tests / n_samples,
                        tests / (t_render * 1e-3), t_host, "equal" if same else "DIFFER from"))
        print(lines[-1], flush=True)
        emit()
    print(emit())


if __name__ == "__main__":
    main()
