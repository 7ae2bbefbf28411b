"""Runs the REFERENCE's mesh simplifier (src_convonet/utils/libsimplify: simplify_mesh.pyx over Simplify.h) on the cases of
tests/simplify_cases.py and stores its output meshes in tests/golden/mesh_simplify_reference.npz (authoring container
only, never on the GPU box).

The reference's module is cythonized and compiled into a temporary directory outside the repository and imported from
there; nothing compiled and no reference source enters the tree.  Needs Cython and a C++ compiler; trimesh is not needed
for mesh_simplify.

    python tests/golden/make_golden_simplify.py [--time]

--time also prints the reference's seconds per case on this host's CPU, and on the 128^3 and 256^3 meshes of
tools/time_simplify.py (profiles/mesh_simplify_timing.md).
"""
import importlib.util
import os
import subprocess
import sys
import sysconfig
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.ref_import import REG_SLICES  # noqa: E402
import simplify_cases  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def build_reference(tmp):
    """-> the reference's compiled simplify_mesh module, built under `tmp`."""
    src = os.path.join(REG_SLICES, "src_convonet", "utils", "libsimplify")
    cpp = os.path.join(tmp, "simplify_mesh.cpp")
    subprocess.run([sys.executable, "-m", "cython", "--cplus", "-3", os.path.join(src, "simplify_mesh.pyx"), "-o", cpp],
                   check=True)
    so = os.path.join(tmp, "simplify_mesh" + sysconfig.get_config_var("EXT_SUFFIX"))
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-w", "-I", src, "-I", sysconfig.get_paths()["include"], "-I",
                    np.get_include(), cpp, "-o", so], check=True)
    spec = importlib.util.spec_from_file_location("simplify_mesh", so)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    timing = "--time" in sys.argv[1:]
    rec = {}
    with tempfile.TemporaryDirectory() as tmp:
        assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
        ref = build_reference(tmp)
        for name, t in simplify_cases.golden_cases():
            v, f = simplify_cases.mesh(name)
            v = np.ascontiguousarray(v, dtype=np.float64)
            f = np.ascontiguousarray(f, dtype=np.int64)
            t0 = time.perf_counter()
            vo, fo = ref.mesh_simplify(v, f, t, simplify_cases.AGGRESSIVENESS)
            dt = time.perf_counter() - t0
            rec["%s_%d_v" % (name, t)], rec["%s_%d_f" % (name, t)] = vo, fo
            print("%-12s F=%6d T=%6d -> V=%6d F=%6d%s" % (name, len(f), t, len(vo), len(fo),
                                                         "  %.4f s" % dt if timing else ""))
        if timing:     # the large meshes of tools/time_simplify.py (host marching cubes gives the device's bits); not stored
            from slice3d_amd.mesh import marching_cubes
            for n in (128, 256):
                v, f = marching_cubes(np.pad(simplify_cases.genus1_field(n), 1, "constant", constant_values=-1e6), 0.0)
                v = np.ascontiguousarray(simplify_cases.genus1_transform(v, n))
                for t in (len(f) // 10, 10000):
                    t0 = time.perf_counter()
                    vo, fo = ref.mesh_simplify(v, f, t, simplify_cases.AGGRESSIVENESS)
                    print("genus1_%-5d F=%7d T=%6d -> V=%6d F=%6d  %.4f s" % (n, len(f), t, len(vo), len(fo),
                                                                             time.perf_counter() - t0))
    path = os.path.join(OUT, "mesh_simplify_reference.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
