"""The input view and the 12 slice images of a mesh, rendered on the device: what `00_img_input/<shape>/<view>.png` and
`01_img_slices/<shape>/<view>/{X,Y,Z}_{1..4}.png` are made from when there is no Blender.

The reference renders these files with Blender (render_slices/blender_script_input.py, blender_script_slices.py).  This
module is not a Cycles clone: the geometry — which pixel shows which part of the object — follows the projection the
models sample their feature pyramids with (datasets.camera_matrices), the slabs follow the reference's 4 x 3 cuts of the
bounding box, and the shading is a documented two-sided Lambert term, 0.8 grey * (0.5 + 0.5 |n.d|).  How checkpoints
trained on Blender images respond to these images has not been measured: the purpose is training on your own meshes.

    SliceRenderer(mesh).render(az, el, distance, ...)   (13, size, size, 4) uint8: view, X_1..X_4, Y_1..Y_4, Z_1..Z_4
    IMAGE_NAMES                                          the 13 names in that order
    make_meta(n_views, seed, size)                       the 7-item meta.pkl list of blender_script_input.py:262-290
    write_shape(renderer, dir_dataset, shape, meta)      the PNGs of one shape under both directories, and meta.pkl

The mesh is in the frame of its 02_sdfs points (mesh_sdf.make_sdf_file, reg_slices/make_sdfs.py).  Meshes are accepted
in the forms of slice3d_amd.mesh_eval; device meshes give device tensors, host meshes numpy arrays.  There is no host
fall-back: the images are computed on the GPU (csrc/mesh_render.hip).
"""
import ctypes as C
import os
import pickle

import numpy as np

from .datasets import blender_proj, camera_matrices
from .mesh_eval import _dev, _device_of, _is_device, _lib, _mesh_arrays, _torch

__all__ = ["SliceRenderer", "IMAGE_NAMES", "make_meta", "write_shape", "camera_frame", "slab_frame", "default_tile"]

IMAGE_NAMES = ("view",) + tuple("%s_%d" % (a, k) for a in "XYZ" for k in (1, 2, 3, 4))
SIZE_MAX = 1024
FOCAL = 35.0 / 32.0


def camera_frame(az, el, distance, offset=(0.0, 0.0, 0.0)):
    """(R (3,3), t (3,)) of a view with meta values az, el, distance, offset: c = (v * scale + t) @ R is the
    object-centred, camera-oriented frame (x right, y down, z away from the camera) — R is the matrix Slice3DDataset
    hands to the model as obj_rot_mat, t its (ox, oz, -oy)."""
    R, _ = camera_matrices(-float(az), float(el), float(distance))
    ox, oy, oz = (float(x) for x in offset)
    return np.ascontiguousarray(R, dtype=np.float64), np.array([ox, oz, -oy], dtype=np.float64)


def slab_frame(R, slice_direction="camera"):
    """The 3 x 4 slab frame M on the c frame.  "camera": the identity — X left to right, Y top to bottom, Z near to
    far.  "axis": the object's axes in the Blender-world mapping that offset_ = (ox, oz, -oy) implies: X = mesh x
    ascending, Y = mesh z ascending, Z = mesh y descending, i.e. rows 0, 2, -1 of R^-1 (as c = w @ R, w = c @ R^-1)."""
    M = np.zeros((3, 4), dtype=np.float64)
    if slice_direction == "camera":
        M[:, :3] = np.eye(3)
    elif slice_direction == "axis":
        Ri = np.linalg.inv(np.asarray(R, dtype=np.float64))
        M[0, :3], M[1, :3], M[2, :3] = Ri[:, 0], Ri[:, 2], -Ri[:, 1]
    else:
        raise ValueError("slice_direction must be 'camera' or 'axis', got %r" % (slice_direction,))
    return M


def default_tile(samples):
    """Pixels per tile edge that give a 256-thread workgroup: 16 / samples."""
    return max(1, 16 // int(samples))


class SliceRenderer:
    """Keeps `mesh` on the device; `render` may run for many cameras."""

    def __init__(self, mesh):
        torch = _torch()
        v, f = _mesh_arrays(mesh)
        self.device = _device_of(v, f)
        self._on_device = _is_device(v) or _is_device(f)
        self._v = _dev(v, torch.float64, self.device).reshape(-1, 3)
        self._f = _dev(f, torch.int64, self.device).reshape(-1, 3)
        self.n_vertices, self.n_faces = self._v.shape[0], self._f.shape[0]
        if self.n_faces == 0 or self.n_vertices == 0:
            raise ValueError("SliceRenderer: the mesh has no face")
        self._L, self._lib = _lib()
        self.n_tests = torch.zeros((), dtype=torch.int64, device=self.device)
        self.n_entries = 0

    def render(self, az, el, distance, scale=1.0, offset=(0.0, 0.0, 0.0), size=256, samples=4, slice_direction="camera",
               vertex_colors=None, return_samples=False, tile=None, resolve=True):
        """The 13 RGBA images (13, size, size, 4) uint8 of one view, in the order of IMAGE_NAMES; with return_samples also
        the per-sample depth (float64, inf = miss) and face (int32, -1 = miss), each (13, size * samples, size * samples).
        `tile` (pixels per tile edge, tile * samples <= 32) changes the speed only.  `vertex_colors` (V, 3) in [0, 1]
        colours the view (image 0), flat per face; the slices stay 0.8 grey.  resolve=False skips the images (timing)."""
        torch = _torch()
        L, lib = self._L, self._lib
        size, samples = int(size), int(samples)
        tile = default_tile(samples) if tile is None else int(tile)
        if not 1 <= size <= SIZE_MAX:
            raise ValueError("size %d outside [1, %d]" % (size, SIZE_MAX))
        if samples not in (1, 2, 4):
            raise ValueError("samples must be 1, 2 or 4, got %d" % samples)
        if tile < 1 or tile * samples > 32:
            raise ValueError("tile %d outside [1, %d] at %d samples" % (tile, 32 // samples, samples))
        if not np.isfinite([float(az), float(el), float(distance), float(scale)]).all():
            raise ValueError("camera values must be finite")
        R, t = camera_frame(az, el, distance, offset)
        M = slab_frame(R, slice_direction)
        cam = np.concatenate([R.reshape(-1), [float(distance), float(scale)], t, M.reshape(-1)]).astype(np.float64)
        if not np.isfinite(cam).all():
            raise ValueError("camera values must be finite")
        colors = None
        if vertex_colors is not None:
            colors = _dev(vertex_colors, torch.float64, self.device)
            if tuple(colors.shape) != (self.n_vertices, 3):
                raise ValueError("vertex_colors must have shape (%d, 3), got %s" % (self.n_vertices, tuple(colors.shape)))
        nb = lib.s3d_mesh_render_workspace_bytes(self.n_vertices, self.n_faces, size, samples, tile)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=self.device)
        st = L.stream_ptr(self.device)
        n = C.c_long(0)
        cam_c = (C.c_double * 26)(*cam.tolist())
        L.check(lib.s3d_mesh_render_build(self._v.data_ptr(), self.n_vertices, self._f.data_ptr(), self.n_faces, cam_c, size,
                                          samples, tile, ws.data_ptr(), nb, C.byref(n), st), "s3d_mesh_render_build")
        self.n_entries = n.value
        entries = torch.empty(max(n.value, 1), dtype=torch.int32, device=self.device)
        L.check(lib.s3d_mesh_render_fill(self.n_vertices, self.n_faces, size, samples, tile, ws.data_ptr(), nb,
                                         entries.data_ptr(), n.value, st), "s3d_mesh_render_fill")
        W = size * samples
        face = torch.empty((13, W, W), dtype=torch.int32, device=self.device)
        depth = torch.empty((13, W, W), dtype=torch.float64, device=self.device) if return_samples else None
        rgba = torch.empty((13, size, size, 4), dtype=torch.uint8, device=self.device) if resolve else None
        nt = torch.empty((), dtype=torch.int64, device=self.device)
        L.check(lib.s3d_mesh_render_render(self.n_vertices, self._f.data_ptr(), self.n_faces, size, samples, tile,
                                           ws.data_ptr(), nb, entries.data_ptr(), n.value,
                                           colors.data_ptr() if colors is not None else None,
                                           depth.data_ptr() if depth is not None else None, face.data_ptr(),
                                           rgba.data_ptr() if rgba is not None else None, nt.data_ptr(), st),
                "s3d_mesh_render_render")
        self.n_tests = nt
        out = tuple(x for x in ((rgba,) + ((depth, face) if return_samples else ())) if x is not None)
        if not self._on_device:
            out = tuple(x.cpu().numpy() for x in out)
        return out if return_samples or not resolve else out[0]


def make_meta(n_views, seed, size=256):
    """The 7-item list that blender_script_input.py:262-290 pickles as meta.pkl, camera_type 'random':
    [K, azimuths, elevations, distances, cam_poses, scale, offset].  K is get_calibration_matrix_K_from_blender's float32
    matrix for a 35 mm lens on a 32 mm sensor at size x size pixels; azimuths = arange(n) / n * 2 pi (float32); elevations
    uniform in [-10, 40] degrees, in radians; distances 1.2; scale uniform in [0.75, 1.1); offset zeros (the reference's
    default, apply_offset off).  cam_poses (n, 3, 4) holds datasets.blender_proj(-az, el, d)[1], the world-to-camera
    matrix of the chain Slice3DDataset rebuilds from az / el / distance; the dataset never reads this item (Blender's own
    matrix_world inverse is not reproduced).  All draws come from np.random.default_rng(seed): elevations first, then the
    scale."""
    n = int(n_views)
    rng = np.random.default_rng(seed)
    f = 35.0 * size / 32.0
    K = np.asarray(((f, 0, size / 2.0), (0, f, size / 2.0), (0, 0, 1)), np.float32)
    az = (np.arange(n) / n * np.pi * 2).astype(np.float32)
    el = np.deg2rad(rng.uniform(-10.0, 40.0, n))
    dist = np.asarray([1.2 for _ in range(n)])
    scale = float(rng.uniform(0.75, 1.1))
    poses = np.stack([blender_proj(-float(az[i]), float(el[i]), float(dist[i]))[1] for i in range(n)], 0) if n else \
        np.zeros((0, 3, 4))
    return [K, az, el, dist, poses, scale, np.zeros(3)]


def write_shape(renderer, dir_dataset, shape, meta, size=256, samples=4, slice_direction="camera", vertex_colors=None,
                tile=None):
    """Renders every view of `meta` and writes `<dir_dataset>/00_img_input/<shape>/<view:03d>.png`,
    `<dir_dataset>/01_img_slices/<shape>/<view:03d>/{X,Y,Z}_{1..4}.png` and, unless it exists, `00_img_input/<shape>/meta.pkl`
    (an existing meta.pkl is never overwritten).  Returns the number of views."""
    from PIL import Image
    dir_ipt = os.path.join(dir_dataset, "00_img_input", shape)
    os.makedirs(dir_ipt, exist_ok=True)
    n = len(meta[1])
    for view in range(n):
        imgs = renderer.render(meta[1][view], meta[2][view], meta[3][view], scale=meta[5], offset=meta[6], size=size,
                               samples=samples, slice_direction=slice_direction, vertex_colors=vertex_colors, tile=tile)
        imgs = imgs.cpu().numpy() if _is_device(imgs) else imgs
        Image.fromarray(imgs[0], "RGBA").save(os.path.join(dir_ipt, "%03d.png" % view))
        d = os.path.join(dir_dataset, "01_img_slices", shape, "%03d" % view)
        os.makedirs(d, exist_ok=True)
        for k in range(1, 13):
            Image.fromarray(imgs[k], "RGBA").save(os.path.join(d, IMAGE_NAMES[k] + ".png"))
    path = os.path.join(dir_ipt, "meta.pkl")
    if not os.path.isfile(path):
        with open(path, "wb") as fh:
            pickle.dump(meta, fh)
    return n
