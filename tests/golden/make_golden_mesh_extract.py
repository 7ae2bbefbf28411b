"""Generates tests/golden/mesh_extract_reference.npz: the case tables of tests/mesh_extract_cases.py run through the
REFERENCE's compiled mesh utilities alone (oracle/_ref, built by `make -C oracle`: libmcubes' marching_cubes template
behind oracle/mc_ref_driver.cpp, and libmise).  Inputs are not stored; every consumer regenerates them from the case
module.  Run from the repo root; `--check` compares a fresh run with the committed file instead of writing it.

  mc/<id>/v, mc/<id>/t        vertices (V,3) float64 and faces (F,3) int64 of the (padded, widened) volume
  mc/<id>/counts, /sha256     the large case: [V, F] and sha256(v bytes, t bytes)
  mise/<id>/q, /qn            every round's queried linear indices, sorted, concatenated (int32); per-round counts
  mise/<id>/dense             the final dense grid
  mise/<id>/qsha, /dsha       the r1 = 65 case: per-round sha256 of the sorted int32 index set, sha256 of the dense grid"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle", "_ref"))

import mesh_extract_cases as K                      # noqa: E402
from make_golden_mesh import ref_marching_cubes     # noqa: E402

OUT = os.path.join(HERE, "mesh_extract_reference.npz")


def mc_record(case):
    v, t = ref_marching_cubes(K.mc_reference_input(case), case.iso)
    if case.digest_only:
        return {"counts": np.array([len(v), len(t)], dtype=np.int64), "sha256": K.sha256_u8(v, t)}
    return {"v": v, "t": t}


def mise_record(case):
    from mise import MISE                           # the compiled reference extension
    rounds, dense = K.drive_host_style(case, MISE(case.r0, case.depth, case.thr))
    sets = [np.sort(q).astype(np.int32) for q in rounds]
    rec = {"qn": np.array([len(s) for s in sets], dtype=np.int64)}
    if case.digest_only:
        rec["qsha"] = np.stack([K.sha256_u8(s) for s in sets])
        rec["dsha"] = K.sha256_u8(dense)
    else:
        rec["q"] = np.concatenate(sets)
        rec["dense"] = dense
    return rec


def records():
    rec = {}
    for case in K.MC_CASES:
        if case.golden == case.id:
            rec.update({"mc/%s/%s" % (case.id, k): a for k, a in mc_record(case).items()})
    for case in K.MISE_CASES:
        rec.update({"mise/%s/%s" % (case.id, k): a for k, a in mise_record(case).items()})
    return rec


def main():
    from helpers import golden_digest
    rec = records()
    if "--check" in sys.argv:
        z = np.load(OUT)
        old = {k: z[k] for k in z.files}
        same = golden_digest(old) == golden_digest(rec)
        print("committed %s\nfresh     %s\n%s" % (golden_digest(old), golden_digest(rec), "identical" if same else "DIFFERENT"))
        return 0 if same else 1
    np.savez_compressed(OUT, **rec)
    print("%d arrays, digest %s, %.1f KB" % (len(rec), golden_digest(rec), os.path.getsize(OUT) / 1024))
    return 0


if __name__ == "__main__":
    sys.exit(main())
