"""Bit digest of the training steps through the C ABI, for comparing two builds of the library.

    python tools/train_step_digest.py [--cases R3,R6,G2] [--out digest.json] [--dump grads.npz]
    python tools/train_step_digest.py --compare parent.json new.json [--dumps parent.npz new.npz]

Each case of CASES runs twice from identical state (weights, BatchNorm running statistics, dropout seed, batch).  For every
tensor (losses, sdf_pred, slices_rec, vgg_loss where the entry point returns it, every parameter gradient by name, every
BatchNorm running statistic after the step) the digest holds the sha256 of the first run and `repeatable`: whether the second
run gave the same bits.  A tensor that is not repeatable (a gradient behind the float-atomic sampling backward) also gets
`self_rel_l2`, the relative L2 difference of its two runs, and --dump keeps its first run for --compare.

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


def rel_l2(a, b):
    d, n = float((a.double() - b.double()).norm()), float(a.double().norm())
    return d / n if n > 0 else d


def digest(names, dump):
    import numpy as np
    import torch  # noqa: F401  (before the library is loaded, so that both use the one HIP runtime torch brings)
    from slice3d_amd import _lib
    res ={"lib": _lib.LIB_PATH, "version": int(_lib.load().s3d_version()), "cases": {}}
    kept = {}
    for name in names:
        tensors = {}
        for k, (a, b) in run_case(name).items():
            bits = a.numpy().tobytes()
            e = {"sha256": hashlib.sha256(bits).hexdigest(), "repeatable": bits == b.numpy().tobytes()}
            if not e["repeatable"]:
                e["self_rel_l2"] = rel_l2(a, b)
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
        for k in ta:
            if k in both:
                continue
            key = name + "/" + k
            cross = rel_l2(torch.from_numpy(da[key]), torch.from_numpy(db[key])) if key in da and key in db else float("nan")
            print("    %s  rel L2 between the libraries %.2e, between the first library's two runs %.2e"
                  % (key, cross, ta[k].get("self_rel_l2", 0.0)))
    print("RESULT: %s" % ("every tensor repeatable in both has the same sha256" if not bad else "%d VIOLATIONS" % bad))
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", help="also write the JSON object to this file")
    ap.add_argument("--dump", help="npz of the first run of every tensor that is not repeatable")
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"))
    ap.add_argument("--dumps", nargs=2, metavar=("A.npz", "B.npz"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(1 if compare(a.compare[0], a.compare[1], a.dumps) else 0)
    res = digest([c for c in a.cases.split(",") if c], a.dump)
    line = json.dumps(res, sort_keys=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
