"""Signed-distance training targets from a triangle mesh on the device: what `02_sdfs/<shape>.npy` is made from.

The reference ships no program for these files (its README points to an external CPU script); the consumer that fixes
their format is Slice3DDataset (slice3d_amd/datasets.py, the reference's reg_slices/src/datasets.py:142-148): float32
`(N, 4)` rows `(x, y, z, signed distance + 0.003)`.

    MeshDistance(mesh).query(points)    exact distance to the nearest point of the mesh (csrc/mesh_sdf.hip)
    winding_number(mesh, points)        generalised winding number
    signed_distance(mesh, points, sign) negative inside; "inside" by ray parity (mesh_eval.MeshIntersector, the
                                        reference's check_mesh_contains bit for bit) or by winding number > 0.5
    sample_sdf_points / make_sdf_file   the query points of a training file, and the file
    normalize_mesh                      bounding box centred on 0, body diagonal 1

Meshes and points are accepted in the forms of slice3d_amd.mesh_eval: numpy arrays or CUDA tensors, `(vertices, faces)`
pairs or objects with `.vertices` / `.faces`.  Device inputs give device results, host inputs numpy results.  There is
no host fall-back: distances, winding numbers and parities are computed on the GPU.
"""
import ctypes as C
import math

import numpy as np

from .mesh_eval import (MeshIntersector, _dev, _device_of, _host, _is_device, _lib, _mesh_arrays, _points3, _torch,
                        sample_surface)

__all__ = ["MeshDistance", "winding_number", "signed_distance", "sample_sdf_points", "make_sdf_file", "normalize_mesh",
           "default_resolution", "SDF_LEVEL"]

SDF_LEVEL = 0.003          # "the sdfs were extracted at the level of 0.003" (datasets.py:144 of the reference)
RES_MAX = 256


def default_resolution(n_faces):
    """Cells per axis of the distance grid for a mesh of `n_faces` faces: a surface of F faces crosses about res^2 cells,
    so res = sqrt(F / 4) leaves a handful of faces in each occupied cell; clamped to [4, 128] (128^3 cells = 36 MB of
    tables)."""
    return int(min(128, max(4, round(math.sqrt(max(int(n_faces), 1) / 4.0)))))


def _points_any(points, device):
    """(n, 3) device tensor of the points' own float width (float32 stays float32, anything else becomes float64)."""
    torch = _torch()
    p = points if _is_device(points) else np.asarray(points)
    f32 = p.dtype == (torch.float32 if _is_device(p) else np.float32)
    return _points3(p, torch.float32 if f32 else torch.float64, device)


class MeshDistance:
    """Exact unsigned distance from points to a triangle mesh.  The cell grid of `mesh` is built once; `query(points)`
    may run many times.  `resolution` (cells per axis, 1..256) changes the speed only: distances and faces are the same
    bits for every value.  After each query `n_tests` holds the number of point-triangle tests as a 0-d device tensor."""

    def __init__(self, mesh, resolution=None):
        torch = _torch()
        v, f = _mesh_arrays(mesh)
        self.device = _device_of(v, f)
        self._v = _dev(v, torch.float64, self.device).reshape(-1, 3)
        self._f = _dev(f, torch.int64, self.device).reshape(-1, 3)
        self.n_faces = self._f.shape[0]
        self.resolution = default_resolution(self.n_faces) if resolution is None else int(resolution)
        L, lib = _lib()
        self._L, self._lib = L, lib
        if not 1 <= self.resolution <= RES_MAX:
            raise ValueError("resolution %d outside [1, %d]" % (self.resolution, RES_MAX))
        if self.n_faces == 0:
            raise ValueError("MeshDistance: the mesh has no face")
        nb = lib.s3d_mesh_dist_workspace_bytes(self.n_faces, self.resolution)
        self._ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
        st = L.stream_ptr(self.device)
        n = C.c_long(0)
        L.check(lib.s3d_mesh_dist_build(self._v.data_ptr(), self._v.shape[0], self._f.data_ptr(), self.n_faces,
                                        self.resolution, self._ws.data_ptr(), nb, C.byref(n), st), "s3d_mesh_dist_build")
        self.n_entries = n.value
        self._entries = torch.empty(max(n.value, 1), dtype=torch.int32, device=self.device)
        L.check(lib.s3d_mesh_dist_fill(self.n_faces, self.resolution, self._ws.data_ptr(), nb, self._entries.data_ptr(),
                                       n.value, st), "s3d_mesh_dist_fill")
        self.n_tests = torch.zeros((), dtype=torch.int64, device=self.device)

    def query(self, points, return_face=False):
        """dist (n,) float64, and with return_face the int64 index of the face that attains it (the lowest on ties)."""
        torch = _torch()
        pts = _points_any(points, self.device)
        n = pts.shape[0]
        dist = torch.empty(n, dtype=torch.float64, device=self.device)
        face = torch.empty(n, dtype=torch.int64, device=self.device) if return_face else None
        nt = torch.empty((), dtype=torch.int64, device=self.device)
        self._L.check(self._lib.s3d_mesh_dist_query(
            self.n_faces, self.resolution, self._ws.data_ptr(), self._ws.numel(), self._entries.data_ptr(), self.n_entries,
            pts.data_ptr(), 1 if pts.dtype == torch.float64 else 0, n, dist.data_ptr(),
            face.data_ptr() if return_face else None, nt.data_ptr(), self._L.stream_ptr(self.device)),
            "s3d_mesh_dist_query")
        self.n_tests = nt
        dist = _host(dist, points)
        return (dist, _host(face, points)) if return_face else dist


def winding_number(mesh, points, n_splits=0):
    """Generalised winding number (n,) float64 of `points` about `mesh`: 1 inside a closed mesh whose faces are
    counter-clockwise seen from outside, 0 outside, in between near a hole.  `n_splits` (0 = automatic) only changes how
    the faces are dealt to blocks, never a bit of the result."""
    torch = _torch()
    v, f = _mesh_arrays(mesh)
    device = _device_of(v, f, points)
    vd = _dev(v, torch.float64, device).reshape(-1, 3)
    fd = _dev(f, torch.int64, device).reshape(-1, 3)
    pts = _points_any(points, device)
    L, lib = _lib()
    n = pts.shape[0]
    w = torch.empty(n, dtype=torch.float64, device=device)
    nws = lib.s3d_mesh_winding_workspace_bytes(fd.shape[0], n)
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=device)
    L.check(lib.s3d_mesh_winding(vd.data_ptr(), vd.shape[0], fd.data_ptr(), fd.shape[0], pts.data_ptr(),
                                 1 if pts.dtype == torch.float64 else 0, n, int(n_splits), ws.data_ptr(), nws, w.data_ptr(),
                                 L.stream_ptr(device)), "s3d_mesh_winding")
    return _host(w, points)


def _inside(mesh, points, sign):
    """Boolean occupancy as a device tensor, by the chosen definition of "inside"."""
    torch = _torch()
    v, f = _mesh_arrays(mesh)
    device = _device_of(v, f, points)
    pts = _points_any(points, device)
    if sign == "parity":
        return MeshIntersector(mesh).query(pts)
    if sign == "winding":
        return winding_number((_dev(v, torch.float64, device), _dev(f, torch.int64, device)), pts) > 0.5
    raise ValueError("sign must be 'parity' or 'winding', got %r" % (sign,))


def signed_distance(mesh, points, sign="parity", resolution=None):
    """Signed distance (n,) float64, negative inside.  The magnitude is MeshDistance's; the sign is one of two
    definitions of "inside", not two implementations of one:
      "parity":  mesh_eval.MeshIntersector — the reference's check_mesh_contains bit for bit, what eval_iou scores with;
                 on a mesh that is not watertight it answers noise;
      "winding": generalised winding number > 0.5, which still means something on an open mesh."""
    torch = _torch()
    v, f = _mesh_arrays(mesh)
    device = _device_of(v, f, points)
    pts = _points_any(points, device)
    inside = _inside(mesh, pts, sign)
    dist = MeshDistance((_dev(v, torch.float64, device), _dev(f, torch.int64, device)), resolution).query(pts)
    return _host(torch.where(inside, -dist, dist), points)


def normalize_mesh(vertices):
    """Vertices moved so that their bounding box is centred on 0 and scaled so that its body diagonal is 1 (the
    normalisation of the reference's README).  numpy in, float64 numpy out; a single point is only centred."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    diag = float(np.linalg.norm(hi - lo))
    return (v - 0.5 * (lo + hi)) / (diag if diag > 0 else 1.0)


def sample_sdf_points(mesh, n, seed, surface_share=0.75, sigmas=(0.0025, 0.01), box=1.0, surface_samples=None):
    """The n query points (n, 3) float64 (host) of a training file: `round(surface_share * n)` surface samples
    (mesh_eval.sample_surface with this seed, or `surface_samples` (>= that many, 3) when given) each displaced by an
    isotropic normal offset — the first half with sigmas[0], the rest with sigmas[1], in units of the bounding-box
    diagonal — followed by points uniform in the cube of side `box` around the bounding-box centre.

    Offsets and uniform points are drawn on the host from np.random.default_rng(seed) (normal offsets first, then the
    uniform points), so the result is a pure function of (mesh, n, seed) given the surface samples, and no device
    random numbers are involved.  The defaults are a starting recipe in the spirit of DeepSDF-style samplers (most
    points near the surface at two scales, the rest filling the cube); they have not been tuned or measured against the
    reference's own training files."""
    v, f = _mesh_arrays(mesh)
    vn = v.detach().cpu().numpy() if _is_device(v) else np.asarray(v)
    fn = f.detach().cpu().numpy() if _is_device(f) else np.asarray(f)
    used = vn.reshape(-1, 3)[fn.reshape(-1)].astype(np.float64)
    lo, hi = used.min(axis=0), used.max(axis=0)
    diag = float(np.linalg.norm(hi - lo))
    n = int(n)
    n_surf = min(n, max(0, int(round(surface_share * n))))
    rng = np.random.default_rng(seed)
    if n_surf:
        if surface_samples is None:
            surface_samples = sample_surface(mesh, n_surf, seed=seed)[0]
        s = surface_samples.detach().cpu().numpy() if _is_device(surface_samples) else np.asarray(surface_samples)
        if s.shape[0] < n_surf:
            raise ValueError("need %d surface samples, got %d" % (n_surf, s.shape[0]))
        sigma = np.full((n_surf, 1), sigmas[1] * diag)
        sigma[: n_surf // 2] = sigmas[0] * diag
        near = s[:n_surf].astype(np.float64) + rng.standard_normal((n_surf, 3)) * sigma
    else:
        near = np.zeros((0, 3))
    uniform = 0.5 * (lo + hi) + rng.uniform(-0.5 * box, 0.5 * box, (n - n_surf, 3))
    return np.concatenate([near, uniform], axis=0)


def make_sdf_file(mesh, path, n, seed, sign="parity", level=SDF_LEVEL, sdf_fn=None, points=None):
    """Writes `path` (.npy): float32 (n, 4) rows (x, y, z, signed distance + level), the reference's on-disk convention
    — Slice3DDataset computes (v - 0.003) * scale and so recovers the true signed distance.  The sign and the distance are
    computed from the float32 points that are written, not from their float64 parents, so what the file says is true of
    what the file holds.  `sdf_fn(mesh, points32)` replaces signed_distance (tests inject a host reference), `points`
    replaces sample_sdf_points.  Returns the array."""
    pts = sample_sdf_points(mesh, n, seed) if points is None else np.asarray(points)
    p32 = np.ascontiguousarray(pts, dtype=np.float32)
    sd = signed_distance(mesh, p32, sign=sign) if sdf_fn is None else sdf_fn(mesh, p32)
    sd = sd.detach().cpu().numpy() if _is_device(sd) else np.asarray(sd)
    out = np.concatenate([p32, (sd.astype(np.float64) + level).astype(np.float32)[:, None]], axis=1)
    np.save(path, out)
    return out
