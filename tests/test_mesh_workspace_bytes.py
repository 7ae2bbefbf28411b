"""The mesh units' *_workspace_bytes functions against the recorded sizes (tests/golden/mesh_workspace_bytes.json, written
by tools/mesh_workspace_sweep.py): workspaces cross calls (build -> fill -> query, run -> emit) and callers allocate by
these numbers, so a layout change that moves one is a change of the C ABI's behaviour.  Host arithmetic: no GPU."""
import ctypes
import json
import os

import pytest

from helpers import GOLDEN
from slice3d_amd import _lib

FUNCTIONS = {"s3d_mesh_contains_workspace_bytes", "s3d_mesh_dist_workspace_bytes", "s3d_mesh_winding_workspace_bytes",
             "s3d_mesh_render_workspace_bytes", "s3d_mesh_simplify_workspace_bytes", "s3d_mesh_topology_workspace_bytes",
             "s3d_nn_workspace_bytes", "s3d_surface_sample_workspace_bytes"}


def test_mesh_workspace_bytes_match_the_recorded_sizes():
    rows = json.load(open(os.path.join(GOLDEN, "mesh_workspace_bytes.json")))
    assert {r[0] for r in rows} == FUNCTIONS
    assert {r[1][2] for r in rows if r[0] == "s3d_mesh_topology_workspace_bytes"} == {0, 1}
    assert sum(1 for r in rows if r[2] == 0) >= 12 and sum(1 for r in rows if r[2] > 0) >= 100
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    try:
        ctypes.CDLL(_lib.LIB_PATH)
    except OSError as e:
        pytest.skip("HIP runtime not loadable here: %s" % e)
    lib = _lib.load()
    got = [[name, args, int(getattr(lib, name)(*args))] for name, args, _ in rows]
    assert [r for r, w in zip(got, rows) if r != w] == []
