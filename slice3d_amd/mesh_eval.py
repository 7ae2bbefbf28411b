"""Mesh evaluation on the device: IoU, Chamfer, F-score, Hausdorff.

Drop-in names and signatures of the reference's scoring helpers (reg_slices/src/utils_eval.py:1-109) and of its
point-in-mesh test (src_convonet/utils/libmesh/inside_mesh.py:5-8), over the kernels of csrc/mesh_eval.hip.

A mesh is a `slice3d_amd.mesh.Mesh`, any object with `.vertices` / `.faces`, or a `(vertices, faces)` pair; arrays are
numpy arrays or CUDA tensors.  Results of device inputs stay on the device; host inputs give numpy results (or Python
floats for the scalar scores).  There is no host fall-back: every score runs on the GPU.
"""
import ctypes as C

import numpy as np

from .mesh import Mesh

__all__ = ["MeshIntersector", "check_mesh_contains", "compute_iou", "eval_iou", "points_dist", "chamfer_dist",
           "eval_chamfer", "eval_hausdoff", "sample_surface", "load_obj"]


def _torch():
    import torch
    return torch


def _device_of(*xs):
    torch = _torch()
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return torch.device("cuda", torch.cuda.current_device())


def _is_device(x):
    torch = _torch()
    return isinstance(x, torch.Tensor) and x.is_cuda


def _dev(x, dtype, device):
    """x (numpy / tensor) as a contiguous device tensor of `dtype` (no copy when it already is one)."""
    torch = _torch()
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device=device, dtype=dtype).contiguous()


def _mesh_arrays(mesh):
    if hasattr(mesh, "vertices") and hasattr(mesh, "faces"):
        return mesh.vertices, mesh.faces
    v, f = mesh
    return v, f


def _points3(p, dtype, device):
    t = _dev(p, dtype, device)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError("points must have shape (n, 3), got %s" % (tuple(t.shape),))
    return t


def _lib():
    from . import _lib as L
    return L, L.load()


def _host(t, like):
    """numpy copy of a device result when the caller's input `like` was a host array, else the tensor itself."""
    return t if _is_device(like) else t.cpu().numpy()


# --------------------------------------------------------------------------------------------------
# point-in-mesh
# --------------------------------------------------------------------------------------------------
class MeshIntersector:
    """inside_mesh.py:11-71 on the device: the cell hash of `mesh` is built once; `query(points)` may run many times.
    `n_disagree` holds, after each query, the number of points inside the bbox whose two ray parities differ (the
    reference prints 'Warning: contains1 != contains2 for some points.' for them) as a 0-d device tensor."""

    def __init__(self, mesh, resolution=512):
        torch = _torch()
        v, f = _mesh_arrays(mesh)
        self.device = _device_of(v, f)
        self.resolution = int(resolution)
        self._v = _dev(v, torch.float64, self.device).reshape(-1, 3)
        self._f = _dev(f, torch.int64, self.device).reshape(-1, 3)
        self.n_faces = self._f.shape[0]
        L, lib = _lib()
        self._L, self._lib = L, lib
        nb = lib.s3d_mesh_contains_workspace_bytes(self.n_faces, self.resolution)
        if nb == 0:
            raise ValueError("hash_resolution %d outside [2, 8192]" % self.resolution)
        self._ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
        st = L.stream_ptr(self.device)
        n = C.c_long(0)
        L.check(lib.s3d_mesh_contains_build(self._v.data_ptr(), self._v.shape[0], self._f.data_ptr(), self.n_faces,
                                            self.resolution, self._ws.data_ptr(), nb, C.byref(n), st),
                "s3d_mesh_contains_build")
        self.n_entries = n.value
        self._entries = torch.empty(max(n.value, 1), dtype=torch.int32, device=self.device)
        L.check(lib.s3d_mesh_contains_fill(self.n_faces, self.resolution, self._ws.data_ptr(), nb,
                                           self._entries.data_ptr(), n.value, st), "s3d_mesh_contains_fill")
        self.n_disagree = torch.zeros((), dtype=torch.int64, device=self.device)

    def query(self, points):
        torch = _torch()
        p = points if _is_device(points) else np.asarray(points)
        f64 = p.dtype == torch.float64 if _is_device(p) else p.dtype == np.float64
        dtype = torch.float64 if f64 else torch.float32
        pts = _points3(p, dtype, self.device)
        inside = torch.empty(pts.shape[0], dtype=torch.bool, device=self.device)
        nd = torch.empty((), dtype=torch.int64, device=self.device)
        self._L.check(self._lib.s3d_mesh_contains_query(
            self.n_faces, self.resolution, self._ws.data_ptr(), self._ws.numel(), self._entries.data_ptr(),
            self.n_entries, pts.data_ptr(), 1 if dtype == torch.float64 else 0, pts.shape[0], inside.data_ptr(), nd.data_ptr(),
            self._L.stream_ptr(self.device)), "s3d_mesh_contains_query")
        self.n_disagree = nd
        if _is_device(points):
            return inside
        if int(nd) > 0:
            print("Warning: contains1 != contains2 for some points.")
        return inside.cpu().numpy()


def check_mesh_contains(mesh, points, hash_resolution=512):
    """Boolean (n,) occupancy of `points` in `mesh`, bit for bit the reference's (inside_mesh.py:5-8)."""
    return MeshIntersector(mesh, hash_resolution).query(points)


# --------------------------------------------------------------------------------------------------
# IoU (utils_eval.py:7-46)
# --------------------------------------------------------------------------------------------------
def _np(x):
    torch = _torch()
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def compute_iou(occ1, occ2):
    """utils_eval.py:7-34 on the host: occupancies thresholded at 0.5, IoU per row; NaN when the union is empty."""
    occ1, occ2 = _np(occ1), _np(occ2)
    if occ1.ndim >= 2:
        occ1 = occ1.reshape(occ1.shape[0], -1)
    if occ2.ndim >= 2:
        occ2 = occ2.reshape(occ2.shape[0], -1)
    occ1 = occ1 >= 0.5
    occ2 = occ2 >= 0.5
    area_union = (occ1 | occ2).astype(np.float32).sum(axis=-1)
    area_intersect = (occ1 & occ2).astype(np.float32).sum(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return area_intersect / area_union


def eval_iou(mesh, qry, occ_tgt):
    """utils_eval.py:36-44: IoU of the mesh's occupancy of `qry` with `occ_tgt`; 0.0 for a mesh with no vertex or face."""
    v, f = _mesh_arrays(mesh)
    if len(v) != 0 and len(f) != 0:
        return compute_iou(check_mesh_contains(mesh, qry), occ_tgt)
    return 0.0


# --------------------------------------------------------------------------------------------------
# nearest neighbours and the distances built on them (utils_eval.py:48-109)
# --------------------------------------------------------------------------------------------------
def nn_sqdist(p1, p2, return_ind=False):
    """Squared distance (float32) from every point of p1 to its nearest point of p2, exact; with return_ind also the
    index (int64, the lowest on ties).  Device tensors in and out."""
    torch = _torch()
    device = _device_of(p1, p2)
    a, b = _points3(p1, torch.float32, device), _points3(p2, torch.float32, device)
    L, lib = _lib()
    na, nb = a.shape[0], b.shape[0]
    d2 = torch.empty(na, dtype=torch.float32, device=device)
    idx = torch.empty(na, dtype=torch.int64, device=device) if return_ind else None
    nws = lib.s3d_nn_workspace_bytes(na)
    ws = torch.empty(nws, dtype=torch.uint8, device=device)
    L.check(lib.s3d_nn_sqdist(a.data_ptr(), na, b.data_ptr(), nb, ws.data_ptr(), nws, d2.data_ptr(),
                              idx.data_ptr() if idx is not None else None, L.stream_ptr(device)), "s3d_nn_sqdist")
    return (d2, idx) if return_ind else d2


def points_dist(p1, p2, k=1, return_ind=False):
    """utils_eval.py:48-55 (cKDTree(p2).query(p1, k)): distance from each point of p1 to its nearest point of p2, and
    its index with return_ind.  Only k = 1 is supported.  Host inputs give float64 / int64 numpy arrays."""
    if k != 1:
        raise ValueError("points_dist: only k=1 is supported, got k=%r" % (k,))
    d2, idx = nn_sqdist(p1, p2, return_ind=True)
    dist = d2.double().sqrt()
    dist, idx = _host(dist, p1), _host(idx, p1)
    return (dist, idx) if return_ind else dist


def chamfer_dist(p1, p2):
    """utils_eval.py:57-60: squared nearest-neighbour distances p1 -> p2 and p2 -> p1 (float64)."""
    d1, d2 = nn_sqdist(p1, p2).double(), nn_sqdist(p2, p1).double()
    return _host(d1, p1), _host(d2, p2)


def eval_chamfer(p1, p2, f_thresh=0.01):
    """utils_eval.py:73-90 -> [chamfer_L1, chamfer_L2, fscore, precision, recall] as Python floats.
    p1: reconstructed points, p2: reference points, (N,3) each.

    fscore is the harmonic mean 2PR/(P+R), 0 when P = R = 0.  The reference's line (utils_eval.py:85,
    `2 * (recall * precision / recall + precision)`) evaluates to 4 * precision, and to NaN when recall is 0."""
    d1, d2 = nn_sqdist(p1, p2).double(), nn_sqdist(p2, p1).double()
    d1s, d2s = d1.sqrt(), d2.sqrt()
    chamfer_l1 = 0.5 * (d1s.mean() + d2s.mean())
    chamfer_l2 = 0.5 * (d1.mean() + d2.mean())
    precision = (d1s < f_thresh).sum().double() / d1.shape[0]
    recall = (d2s < f_thresh).sum().double() / d2.shape[0]
    chamfer_l1, chamfer_l2, precision, recall = (float(x) for x in (chamfer_l1, chamfer_l2, precision, recall))
    fscore = 2.0 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
    return [chamfer_l1, chamfer_l2, fscore, precision, recall]


def eval_hausdoff(p1, p2):
    """utils_eval.py:92-102 (scipy directed_hausdorff both ways) -> (rec->ref, ref->rec, max) as Python floats."""
    d12 = float(nn_sqdist(p1, p2).max().double().sqrt())
    d21 = float(nn_sqdist(p2, p1).max().double().sqrt())
    return d12, d21, max(d12, d21)


# --------------------------------------------------------------------------------------------------
# surface sampling and .obj input
# --------------------------------------------------------------------------------------------------
def sample_surface(mesh, n, seed=0):
    """n area-weighted points on the surface of `mesh` -> (points (n,3) float32, face_idx (n,) int64).  The same seed
    gives the same bits whatever the launch geometry; zero-area faces are never chosen."""
    torch = _torch()
    v, f = _mesh_arrays(mesh)
    device = _device_of(v, f)
    vd = _dev(v, torch.float64, device).reshape(-1, 3)
    fd = _dev(f, torch.int64, device).reshape(-1, 3)
    L, lib = _lib()
    n = int(n)
    pts = torch.empty((n, 3), dtype=torch.float32, device=device)
    fidx = torch.empty(n, dtype=torch.int64, device=device)
    nws = lib.s3d_surface_sample_workspace_bytes(fd.shape[0])
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=device)
    L.check(lib.s3d_surface_sample(vd.data_ptr(), vd.shape[0], fd.data_ptr(), fd.shape[0], n,
                                   int(seed) & 0xFFFFFFFFFFFFFFFF, ws.data_ptr(), nws, pts.data_ptr(), fidx.data_ptr(),
                                   L.stream_ptr(device)), "s3d_surface_sample")
    return _host(pts, v), _host(fidx, v)


def load_obj(path):
    """Wavefront .obj -> Mesh: the `v` and `f` lines (as Mesh.export writes them; `f a/b/c` and negative indices read
    too), polygons fan-triangulated (v0, vi, vi+1)."""
    verts, faces = [], []
    with open(path) as fh:
        for line in fh:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v":
                verts.append([float(x) for x in tok[1:4]])
            elif tok[0] == "f":
                ids = []
                for t in tok[1:]:
                    i = int(t.split("/")[0])
                    ids.append(i - 1 if i > 0 else len(verts) + i)
                for k in range(1, len(ids) - 1):
                    faces.append([ids[0], ids[k], ids[k + 1]])
    return Mesh(np.asarray(verts, dtype=np.float64).reshape(-1, 3), np.asarray(faces, dtype=np.int64).reshape(-1, 3))
