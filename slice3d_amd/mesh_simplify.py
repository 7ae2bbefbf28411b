"""Mesh simplification on the device: quadric edge collapse (csrc/mesh_simplify.hip).

Drop-in names, spellings and defaults of the reference's libsimplify (src_convonet/utils/libsimplify):

    mesh_simplify(vertices, faces, f_target, agressiveness=7.) -> (vertices, faces)      simplify_mesh.pyx
    simplify_mesh(mesh, f_target=10000, agressiveness=7.)      -> Mesh                    libsimplify/__init__.py

Meshes are accepted in the forms of slice3d_amd.mesh_eval: numpy arrays or CUDA tensors, `(vertices, faces)` pairs or
objects with `.vertices` / `.faces`.  Device arrays in give device arrays out, host arrays numpy arrays.  There is no
host fall-back: every collapse runs on the GPU.  `simplify_stats` returns the rounds alongside.
"""
import ctypes as C

import numpy as np

from .mesh import Mesh
from .mesh_eval import _dev, _device_of, _host, _is_device, _lib, _mesh_arrays, _torch

__all__ = ["mesh_simplify", "simplify_mesh", "simplify_stats"]


def simplify_stats(vertices, faces, f_target, agressiveness=7.):
    """-> (vertices (V', 3) float64, faces (F', 3) int64, rounds).  F' is f_target or up to two below it unless the 100
    rounds run out first; vertices that no face references any more are dropped, the others keep their order."""
    torch = _torch()
    if not _is_device(faces) and np.asarray(faces).size == 0:
        return vertices, faces, 0
    if _is_device(faces) and faces.numel() == 0:
        return vertices, faces, 0
    device = _device_of(vertices, faces)
    vd = _dev(vertices, torch.float64, device).reshape(-1, 3)
    fd = _dev(faces, torch.int64, device).reshape(-1, 3)
    L, lib = _lib()
    nv, nf = vd.shape[0], fd.shape[0]
    nb = lib.s3d_mesh_simplify_workspace_bytes(nv, nf)
    if nb == 0:
        raise ValueError("mesh_simplify: %d vertices, %d faces cannot be served" % (nv, nf))
    ws = torch.empty(nb, dtype=torch.uint8, device=device)
    st = L.stream_ptr(device)
    nvo, nfo, rounds = C.c_long(0), C.c_long(0), C.c_int(0)
    L.check(lib.s3d_mesh_simplify_run(vd.data_ptr(), nv, fd.data_ptr(), nf, int(f_target), float(agressiveness),
                                      ws.data_ptr(), nb, C.byref(nvo), C.byref(nfo), C.byref(rounds), st),
            "s3d_mesh_simplify_run")
    vo = torch.empty((nvo.value, 3), dtype=torch.float64, device=device)
    fo = torch.empty((nfo.value, 3), dtype=torch.int64, device=device)
    if nvo.value and nfo.value:
        L.check(lib.s3d_mesh_simplify_emit(ws.data_ptr(), nb, nv, nf, vo.data_ptr(), fo.data_ptr(), st),
                "s3d_mesh_simplify_emit")
    return _host(vo, vertices), _host(fo, faces), rounds.value


def mesh_simplify(vertices, faces, f_target, agressiveness=7.):
    """simplify_mesh.pyx: -> (vertices, faces) with about `f_target` faces."""
    v, f, _ = simplify_stats(vertices, faces, f_target, agressiveness)
    return v, f


def simplify_mesh(mesh, f_target=10000, agressiveness=7.):
    """libsimplify/__init__.py: -> Mesh with about `f_target` faces.  An empty mesh is returned as it is."""
    v, f = _mesh_arrays(mesh)
    if (f.numel() if _is_device(f) else np.asarray(f).size) == 0:
        return mesh
    vo, fo = mesh_simplify(v, f, f_target, agressiveness)
    if _is_device(vo):
        vo, fo = vo.cpu().numpy(), fo.cpu().numpy()
    return Mesh(vo, fo)
