"""Bit digest of the training steps and of the inference front end through the C ABI, for comparing two builds of the library.

    python tools/train_step_digest.py [--cases R3,R6,G2,I4] [--out digest.json] [--dump grads.npz]
    python tools/train_step_digest.py --compare parent.json new.json [--dumps parent.npz new.npz]

Each case of CASES runs twice from identical state (weights, BatchNorm running statistics, dropout seed, batch).  For every
tensor (losses, sdf_pred, slices_rec, vgg_loss where the entry point returns it, every parameter gradient by name, every
BatchNorm running statistic after the step) the digest holds the sha256 of the first run and `repeatable`: whether the second
run gave the same bits.  A tensor that is not repeatable (a gradient behind the float-atomic sampling backward) also gets
`self_rel_l2`, the relative L2 difference of its two runs, and --dump keeps its first run for --compare (--dump-all: of every
tensor, so that --compare can also say how far apart two repeatable tensors of different bits are).  The cases of
INFER_CASES do the same for the outputs of the decode entry points, the query sort, project_coord and the two samplers.

The library is whatever S3D_HIP_LIB selects (slice3d_amd/_lib.py): run the tool once per build, each in a fresh process.
--compare checks the requirement between two digests: every tensor repeatable in both has the same sha256; exit status 1
otherwise.  Inputs come from make_feed_dict / load_seeded; nothing is read from disk."""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name: (entry, prec, B, S, Q, ns, dropout, options of the split entry)
CASES = {
    "R1": ("fused", "f32", 1, 32, 50, 12, 0.1, None),       # no query sort, atomic sampler backward, vgg_prep path
    "R2": ("fused", "f16x3", 2, 48, 33, 4, 0.0, None),      # S not a power of two, fused VGG first layer
    "R3": ("fused", "f16x3", 2, 32, 5000, 12, 0.1, None),   # sorted queries, atomic-free sampler backward
    "R4": ("fused", "f32", 2, 32, 5000, 12, 0.1, None),     # the same in fp32
    "R5": ("fused", "f16", 2, 32, 5000, 12, 0.1, None),     # the single-pass decoder mode
    "R6": ("split", "f16x3", 2, 32, 5000, 12, 0.1, {"d_rec": True, "d_vgg": 1.0, "grad_scale": 0.0}),
    "R7": ("split", "f16x3", 2, 32, 5000, 12, 0.0, {"d_rec": False, "d_vgg": 0.0, "grad_scale": 1024.0}),
    "G1": ("gt", "f32", 2, 32, 130, 12, 0.1, None),         # no sort
    "G2": ("gt", "f16x3", 1, 32, 4200, 4, 0.0, None),       # sorted queries
}


def run_case(name):
    """{tensor name: [run 0, run 1]} as CPU tensors."""
    import torch
    from slice3d_amd.models import Slices3DRegModel
    from slice3d_amd.models_gt import Slices3DGTModel
    from slice3d_amd.synth import make_feed_dict
    from slice3d_amd.trainer import HipGtTrainer, HipTrainer
    from slice3d_amd.weights import load_seeded
    entry, prec, b, s, q, ns, dropout, opt = CASES[name]
    fd = make_feed_dict(b, s, q, ns, seed=700 + q, device="cuda")
    if entry == "gt":
        m = load_seeded(Slices3DGTModel(n_slices=ns, mode="train"), 0).cuda()
        tr = HipGtTrainer(m, prec=prec, dropout=dropout, seed=11)
    else:
        m = load_seeded(Slices3DRegModel(img_size=s, n_slices=ns, mode="train"), 0).cuda()
        tr = HipTrainer(m, prec=prec, dropout=dropout, seed=11)
    stats0 = {k: v.clone() for k, v in m.state_dict().items() if "running" in k}
    if entry == "split":
        g = torch.Generator().manual_seed(5)
        d_sdf = (torch.randn(b, q, generator=g) / (b * q)).cuda()
        d_rec = (torch.randn(b * ns, 3, s, s, generator=g) / (b * ns * 3 * s * s)).cuda() if opt["d_rec"] else None
    out = {}
    for _ in range(2):
        tr._calls = 0                                 # the same dropout seed for both runs
        m.load_state_dict(stats0, strict=False)       # the step moves the BatchNorm running statistics
        tr.grad_flat.zero_()
        if entry == "fused":
            losses, sdf, rec = tr.forward_backward(fd, want_outputs=True)
            got = {"losses": losses, "sdf_pred": sdf, "slices_rec": rec}
        elif entry == "gt":
            losses, sdf = tr.forward_backward(fd, want_outputs=True)
            got = {"losses": losses, "sdf_pred": sdf}
        else:
            sdf, rec, vgg, ctx = tr.forward_only(fd)
            got = {"sdf_pred": sdf.clone(), "slices_rec": rec.clone(), "vgg_loss": vgg.clone()}
            tr.backward_from(ctx, d_sdf, d_rec, opt["d_vgg"], grad_scale=opt["grad_scale"])
        torch.cuda.synchronize()
        for k, p in zip(tr.names, tr.params):
            off = tr.offsets[k]
            got["grad:" + k] = tr.grad_flat[off:off + p.numel()]
        for k, v in m.state_dict().items():
            if "running" in k:
                got["bn:" + k] = v
        for k, v in got.items():
            out.setdefault(k, []).append(v.detach().float().cpu().clone())
    del tr, m
    torch.cuda.empty_cache()
    return out


# Inference cases: the query front end on the shapes, query / grid sets and per-object cameras of tests/query_cases.py (S = 32).
# name: (kind, prec, B, Q, ns, mode)
INFER_CASES = {
    "I1": ("reg", "f32", 3, 50, 12, "train"),       # caller order (Q < 4096): sdf, fc_p and fc_s rows
    "I2": ("reg", "f16x3", 3, 50, 12, "train"),
    "I3": ("reg", "f32", 2, 4200, 3, "test"),       # locality-sorted, flip
    "I4": ("reg", "f16x3", 2, 4200, 3, "train"),    # locality-sorted, rotation
    "I5": ("grid", "f16x3", 1, 4200, 3, "test"),    # dense grid of 20^3 points, the slab [1234, 1234 + Q)
    "I6": ("gt", "f16x3", 2, 4200, 3, "test"),
    "I7": ("sort", None, 3, 30000, 0, "train"),     # s3d_query_sort: permutation and bin ends
    "I8": ("project", None, 3, 257, 0, "none"),     # s3d_project_coord_fwd: uniform and border sets
    "I9": ("samplers", None, 2, 4097, 3, "none"),   # sample_planes and the pyramid sampler, grids that leave [-1, 1]
}


def run_infer_case(name):
    """{tensor name: [run 0, run 1]} as CPU tensors, like run_case."""
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import query_cases as K
    from slice3d_amd import _lib as L
    from slice3d_amd.models import Slices3DRegModel
    from slice3d_amd.models_gt import Slices3DGTModel
    from slice3d_amd.synth import make_feed_dict
    from slice3d_amd.weights import load_seeded
    kind, prec, b, q, ns, mode = INFER_CASES[name]
    s, lib = 32, L.load()

    def feed(first_cam=0, with_slices=False):
        fd = K.with_cameras(make_feed_dict(b, s, q, ns, seed=600 + q, with_slices=with_slices), K.cams_of(b, first_cam))
        return {k: v.cuda() for k, v in fd.items()}

    def once():
        if kind == "reg":
            m = load_seeded(Slices3DRegModel(n_slices=ns, mode=mode, prec=prec), 0).cuda().eval()
            fd = feed()
            got = {"sdf_pred": m(fd)["sdf_pred"]}
            if q < 4096:
                st = m.decode_stages(fd["qry_norot"], m.encode(fd))
                got.update({"fc_p": st["fc_p"], "fc_s": st["fc_s"], "sdf_stages": st["sdf"]})
            return got
        if kind == "grid":
            m = load_seeded(Slices3DRegModel(n_slices=ns, mode=mode, prec=prec), 0).cuda().eval()
            return {"logits": m.decode_grid(m.encode(feed()), 20, box=1.1, q_range=(1234, 1234 + q))}
        if kind == "gt":
            m = load_seeded(Slices3DGTModel(n_slices=ns, mode=mode, prec=prec), 0).cuda().eval()
            return {"sdf_pred": m(feed(first_cam=1, with_slices=True))["sdf_pred"]}
        if kind == "sort":
            cams = K.cams_of(b)
            rot, trans = K.rot_trans(cams)
            qg, rg, tg = K.sort_camera_inputs(batch=b, q=q).cuda(), rot.cuda(), trans.cuda()
            nbytes = lib.s3d_query_sort_workspace_bytes(b, q)
            ws = torch.empty(nbytes // 4 + 1, dtype=torch.int32, device="cuda")
            got = {}
            for flip in (0, 1):
                perm = torch.empty((b, q), dtype=torch.int32, device="cuda")
                L.check(lib.s3d_query_sort(qg.data_ptr(), rg.data_ptr(), tg.data_ptr(), flip, b, q, perm.data_ptr(), ws.data_ptr(),
                                           nbytes, None), "s3d_query_sort")
                got["perm-flip%d" % flip], got["bin_ends-flip%d" % flip] = perm, ws[:b * 65536].clone()
            return got
        if kind == "project":
            cams = K.cams_of(b)
            tg, got = K.rot_trans(cams)[1].cuda(), {}
            for sname in ("uniform", "border"):
                cg = K.query_set(sname, b, q, 100 + q, cams, mode).cuda()
                out = torch.empty((b, q, 2), dtype=torch.float32, device="cuda")
                L.check(lib.s3d_project_coord_fwd(cg.data_ptr(), tg.data_ptr(), out.data_ptr(), b, q, None), "s3d_project_coord_fwd")
                got["grid-" + sname] = out
            return got
        got = {}
        for h, w, c in K.PLANE_SHAPES[2:]:
            pg = K.planes(3, h, w, c, seed=1000 * h + 10 * w + c).cuda()
            for gname, grid in K.plane_grid_sets(3, 63, w, h, seed=63 + h).items():
                gg, out = grid.cuda(), torch.empty((3, 63, c), dtype=torch.float32, device="cuda")
                L.check(lib.s3d_sample_planes_fwd(pg.data_ptr(), gg.data_ptr(), out.data_ptr(), 3, h, w, c, 63, None), "s3d_sample_planes_fwd")
                got["planes-%dx%dx%d-%s" % (h, w, c, gname)] = out
        m = Slices3DRegModel(img_size=s, n_slices=ns, mode="test").cuda().eval()
        pyr = [p.cuda() for p in K.pyramid(b * ns, s, seed=s + ns)]
        for pq in (129, q):
            for gname in ("uniform", "pile", "walk"):
                got["pyramid-q%d-%s" % (pq, gname)] = m.sample_pyramid(pyr, K.pyramid_grid(gname, b, pq, s, seed=pq + ns).cuda())
        return got

    out = {}
    for _ in range(2):
        with torch.no_grad():
            got = once()
        torch.cuda.synchronize()
        for k, v in got.items():
            out.setdefault(k, []).append(v.detach().cpu().clone())
    torch.cuda.empty_cache()
    return out


def rel_l2(a, b):
    d, n = float((a.double() - b.double()).norm()), float(a.double().norm())
    return d / n if n > 0 else d


def digest(names, dump, dump_all=False):
    import numpy as np
    import torch  # noqa: F401  (before the library is loaded, so that both use the one HIP runtime torch brings)
    from slice3d_amd import _lib
    res ={"lib": _lib.LIB_PATH, "version": int(_lib.load().s3d_version()), "cases": {}}
    kept = {}
    for name in names:
        tensors = {}
        for k, (a, b) in (run_infer_case if name in INFER_CASES else run_case)(name).items():
            bits = a.numpy().tobytes()
            e = {"sha256": hashlib.sha256(bits).hexdigest(), "repeatable": bits == b.numpy().tobytes()}
            if not e["repeatable"]:
                e["self_rel_l2"] = rel_l2(a, b)
            if dump_all or not e["repeatable"]:
                kept[name + "/" + k] = a.numpy()
            tensors[k] = e
        res["cases"][name] = tensors
    if dump:
        np.savez(dump, **kept)
    return res


def compare(pa, pb, dumps):
    """Requirement: a tensor repeatable in both digests has the same sha256 in both.  Prints one line per case and one per
    tensor that is not repeatable; returns the number of violations."""
    import numpy as np
    import torch
    A, B = json.load(open(pa)), json.load(open(pb))
    da, db = (np.load(dumps[0]), np.load(dumps[1])) if dumps else ({}, {})
    bad = 0
    for name in A["cases"]:
        ta, tb = A["cases"][name], B["cases"].get(name)
        if tb is None or set(ta) != set(tb):
            print("%s: the two digests hold different tensors" % name)
            bad += 1
            continue
        both = [k for k in ta if ta[k]["repeatable"] and tb[k]["repeatable"]]
        differ = [k for k in both if ta[k]["sha256"] != tb[k]["sha256"]]
        bad += len(differ)
        print("%s: %d tensors, %d repeatable in both, %d of those differ%s"
              % (name, len(ta), len(both), len(differ), " " + str(differ[:5]) if differ else ""))
        cross_of = lambda key: rel_l2(torch.from_numpy(da[key]), torch.from_numpy(db[key])) if key in da and key in db else float("nan")
        for k in differ:
            print("    %s/%s  repeatable in both, DIFFERENT: rel L2 between the libraries %.2e" % (name, k, cross_of(name + "/" + k)))
        for k in ta:
            if k in both:
                continue
            key = name + "/" + k
            cross = cross_of(key)
            print("    %s  rel L2 between the libraries %.2e, between the first library's two runs %.2e"
                  % (key, cross, ta[k].get("self_rel_l2", 0.0)))
    print("RESULT: %s" % ("every tensor repeatable in both has the same sha256" if not bad else "%d VIOLATIONS" % bad))
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", default=",".join(list(CASES) + list(INFER_CASES)))
    ap.add_argument("--out", help="also write the JSON object to this file")
    ap.add_argument("--dump", help="npz of the first run of every tensor that is not repeatable")
    ap.add_argument("--dump-all", action="store_true", help="--dump keeps the first run of every tensor, repeatable or not")
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"))
    ap.add_argument("--dumps", nargs=2, metavar=("A.npz", "B.npz"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(1 if compare(a.compare[0], a.compare[1], a.dumps) else 0)
    res = digest([c for c in a.cases.split(",") if c], a.dump, a.dump_all)
    line = json.dumps(res, sort_keys=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
