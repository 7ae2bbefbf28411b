"""SHA-256 of every output array of the five mesh units (mesh_eval, mesh_sdf, mesh_render, mesh_simplify, mesh_topology)
on the small fixtures of tests/golden/mesh_eval_reference.npz: one line per array.  Two builds of the library that print the
same lines compute the same bits on these inputs (S3D_HIP_LIB selects the library).  A record for a change that must not
alter results, not a gate: digests of sqrt / atan2 results need not survive a compiler update.

Left out, because the units document them as scheduling-dependent: the order of the entries inside a cell or tile list,
and the topology's round count.

    python tools/mesh_digest.py [--out FILE]
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slice3d_amd import _lib, mesh_eval, mesh_render, mesh_sdf, mesh_simplify, mesh_topology   # noqa: E402

LINES = []


def put(name, x):
    x = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    x = np.ascontiguousarray(x)
    h = hashlib.sha256(("%s %s " % (x.dtype, x.shape)).encode() + x.tobytes()).hexdigest()
    LINES.append("%s %s %s %s" % (h[:32], name, x.dtype, "x".join(str(s) for s in x.shape)))
    print(LINES[-1], flush=True)


def soup(v, f, seed=0):
    """every face gets its own three vertices, shuffled: duplicated positions for the weld"""
    perm = np.random.default_rng(seed).permutation(3 * len(f))
    vs = np.empty((3 * len(f), 3))
    vs[perm] = v[f.reshape(-1)]
    return vs, perm.reshape(-1, 3).astype(np.int64)


def table_arrays(pre, topo):
    for key in sorted(topo.table):
        put("%s.table.%s" % (pre, key), topo.table[key])
    for key in sorted(topo.summary):
        put("%s.summary.%s" % (pre, key), topo.summary[key])


def topology(pre, v, f, weld):
    topo = mesh_topology.mesh_topology((v, f), weld=weld)
    put(pre + ".n_components", np.int64(topo.n_components))
    put(pre + ".face_component", topo.face_component)
    put(pre + ".vertex_component", topo.vertex_component)
    put(pre + ".vmap", topo.vmap)
    table_arrays(pre, topo)
    mask = mesh_topology.select_components(topo.table, largest=1)
    for tag, m, drop in (("largest", mask, False), ("all_drop_degenerate", np.ones_like(mask), True)):
        vo, fo = topo._run.keep(m, drop)
        put("%s.keep_%s.vertices" % (pre, tag), vo)
        put("%s.keep_%s.faces" % (pre, tag), fo)


def one_mesh(name, v, f, pts):
    rng = np.random.default_rng(5)
    lo, hi = v.min(0), v.max(0)
    pts = np.concatenate([pts, rng.uniform(lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo), (2000, 3))])
    for tag, p in (("f64", pts), ("f32", pts.astype(np.float32))):
        for res in (64, 512):
            put("%s.contains%d.%s" % (name, res, tag), mesh_eval.MeshIntersector((v, f), res).query(p))
        for res in (None, 1, 7):
            d, face = mesh_sdf.MeshDistance((v, f), res).query(p, return_face=True)
            put("%s.dist_res%s.%s" % (name, res, tag), d)
            put("%s.dist_face_res%s.%s" % (name, res, tag), face)
        put("%s.winding.%s" % (name, tag), mesh_sdf.winding_number((v, f), p))
        put("%s.winding_split3.%s" % (name, tag), mesh_sdf.winding_number((v, f), p, n_splits=3))
    vn = mesh_sdf.normalize_mesh(v)
    colors = np.random.default_rng(7).uniform(0, 1, (len(v), 3))
    r = mesh_render.SliceRenderer((vn, f))
    for tag, kw in (("camera", dict(size=32, samples=2)), ("axis36", dict(size=36, samples=4, slice_direction="axis")),
                    ("s1_tile5", dict(size=33, samples=1, tile=5))):
        rgba, depth, face = r.render(0.7, 0.3, 1.2, scale=0.9, offset=(0.03, -0.02, 0.04), vertex_colors=colors,
                                     return_samples=True, **kw)
        put("%s.render_%s.rgba" % (name, tag), rgba)
        put("%s.render_%s.depth" % (name, tag), depth)
        put("%s.render_%s.face" % (name, tag), face)
    for ratio in (2, 8):
        vo, fo, _ = mesh_simplify.simplify_stats(v, f, len(f) // ratio)
        put("%s.simplify_%d.vertices" % (name, ratio), vo)
        put("%s.simplify_%d.faces" % (name, ratio), fo)
    topology(name + ".topology", v, f, False)
    sa, fa = mesh_eval.sample_surface((v, f), 5000, seed=1)
    sb, fb = mesh_eval.sample_surface((v, f), 3001, seed=2)
    put(name + ".sample5000.points", sa)
    put(name + ".sample5000.faces", fa)
    put(name + ".sample3001.points", sb)
    d2, idx = mesh_eval.nn_sqdist(_dev(sa), _dev(sb), return_ind=True)
    put(name + ".nn.d2", d2)
    put(name + ".nn.idx", idx)


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def error_path(v, f):
    """a face that names vertex n_vertices: every unit refuses it, with its own message"""
    bad = f.copy()
    bad[len(bad) // 2, 1] = len(v)
    p = v[:10]
    calls = [("contains", lambda: mesh_eval.MeshIntersector((v, bad), 64)),
             ("dist", lambda: mesh_sdf.MeshDistance((v, bad))),
             ("winding", lambda: mesh_sdf.winding_number((v, bad), p)),
             ("render", lambda: mesh_render.SliceRenderer((v, bad)).render(0.7, 0.3, 1.2, size=16, samples=2)),
             ("simplify", lambda: mesh_simplify.simplify_stats(v, bad, 100)),
             ("topology", lambda: mesh_topology.mesh_topology((v, bad))),
             ("topology_weld", lambda: mesh_topology.mesh_topology((v, bad), weld=True))]
    for name, fn in calls:
        try:
            fn()
            msg = "no error"
        except _lib.S3dError as e:
            msg = str(e)
        put("error.%s: %s" % (name, msg), np.frombuffer(msg.encode(), dtype=np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    z = np.load(os.path.join(ROOT, "tests", "golden", "mesh_eval_reference.npz"))
    print("# library: %s" % _lib.LIB_PATH, flush=True)
    for name in ("sphere", "torus", "boxes"):
        one_mesh(name, z[name + "_v"], z[name + "_f"], z[name + "_pts"])
    vs, fs = soup(z["boxes_v"], z["boxes_f"])
    topology("soup.topology_weld", vs, fs, True)
    topology("soup.topology", vs, fs, False)
    wv, wf, wmap = mesh_topology.weld(vs, fs)
    put("soup.weld.vertices", wv)
    put("soup.weld.faces", wf)
    put("soup.weld.vmap", wmap)
    error_path(z["sphere_v"], z["sphere_f"])
    total = hashlib.sha256("\n".join(LINES).encode()).hexdigest()
    print("# %d arrays, digest of the digests: %s" % (len(LINES), total[:32]))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n# %d arrays, digest of the digests: %s\n" % (len(LINES), total[:32]))


if __name__ == "__main__":
    main()
