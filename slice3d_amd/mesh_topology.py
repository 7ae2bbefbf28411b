"""Mesh topology on the device (csrc/mesh_topology.hip): weld of equal positions, connected components, per-component
counts and measures, and the order-preserving removal of components — what the reference asks trimesh for.

    weld(vertices, faces)                      -> (vertices, faces, vmap)
    mesh_topology(mesh, weld=False)            -> MeshTopology
    split(mesh, weld=False)                    -> [Mesh]
    select_components(table, largest=None, by="faces", min_faces=0, min_frac=0.0) -> bool mask     (host code)
    keep_components(mesh, mask_or_rules, drop_degenerate=False, weld=False)      -> Mesh
    largest_component(mesh, by="faces")        -> Mesh

Meshes are accepted in the forms of slice3d_amd.mesh_eval: numpy arrays or CUDA tensors, `(vertices, faces)` pairs or
objects with `.vertices` / `.faces`.  Device arrays in give device arrays out, host arrays numpy arrays; the table is
always numpy.  There is no host fall-back: labels, counts and sums come from the GPU.

Two vertices are welded when their coordinates compare equal as float64 (-0.0 equals +0.0); a class is represented by its
smallest index.  Two faces are connected when they share a (welded) vertex.  Component ids ascend with the component's
smallest vertex index.  The table's columns are COUNT_COLUMNS (int64; the two flags bool) and `area`, `volume`, `bbox`
(float64), defined as tests/simplify_ref.py's edge_face_counts, is_oriented_manifold and euler_characteristic define them
on the component's welded faces.
"""
import ctypes as C

import numpy as np

from .mesh import Mesh
from .mesh_eval import _dev, _device_of, _host, _is_device, _lib, _mesh_arrays, _torch

__all__ = ["COUNT_COLUMNS", "MeshTopology", "weld", "mesh_topology", "split", "select_components", "keep_components",
           "largest_component"]

COUNT_COLUMNS = ("faces", "vertices", "edges", "edges_1", "edges_2", "edges_3plus", "conflicts", "degenerate", "euler",
                 "closed_oriented", "oriented_with_border")
_FLAGS = ("closed_oriented", "oriented_with_border")
N_MEASURES = 8       # area, volume, bbox lo xyz, bbox hi xyz


def table_from_arrays(counts, measures):
    """(n, 11) int64 and (n, 8) float64 rows -> the table: a dict of named numpy columns."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, len(COUNT_COLUMNS))
    measures = np.asarray(measures, dtype=np.float64).reshape(-1, N_MEASURES)
    t = {name: (counts[:, i] != 0) if name in _FLAGS else counts[:, i].copy() for i, name in enumerate(COUNT_COLUMNS)}
    t["area"], t["volume"], t["bbox"] = measures[:, 0].copy(), measures[:, 1].copy(), measures[:, 2:8].copy()
    return t


class MeshTopology:
    """n_components, face_component (F,), vertex_component (V,; -1 for a vertex no face references), vmap (V,; the welded
    representative of every vertex), table (dict of columns, one entry per component), summary (dict of scalars over all
    faces), rounds (hook / compress / check rounds the labels took), is_watertight."""

    def __init__(self, run, like):
        torch = _torch()
        L, lib = _lib()
        self._run = run
        self.n_components, self.rounds, self.welded = run.k, run.rounds, bool(run.weld)
        dev = run.device
        vmap = torch.empty(run.nv, dtype=torch.int64, device=dev)
        fcomp = torch.empty(run.nf, dtype=torch.int64, device=dev)
        vcomp = torch.empty(run.nv, dtype=torch.int64, device=dev)
        L.check(lib.s3d_mesh_topology_emit_labels(run.ws.data_ptr(), run.nb, run.nv, run.nf, run.weld, vmap.data_ptr(),
                                                  fcomp.data_ptr(), vcomp.data_ptr(), run.st), "s3d_mesh_topology_emit_labels")
        counts = torch.empty((run.k + 1, len(COUNT_COLUMNS)), dtype=torch.int64, device=dev)
        measures = torch.empty((run.k + 1, N_MEASURES), dtype=torch.float64, device=dev)
        L.check(lib.s3d_mesh_topology_emit_table(run.ws.data_ptr(), run.nb, run.nv, run.nf, run.weld, run.k,
                                                 counts.data_ptr(), measures.data_ptr(), run.st), "s3d_mesh_topology_emit_table")
        self.vmap, self.face_component, self.vertex_component = _host(vmap, like), _host(fcomp, like), _host(vcomp, like)
        counts, measures = counts.cpu().numpy(), measures.cpu().numpy()
        self.table = table_from_arrays(counts[:-1], measures[:-1])
        self.summary = {k: (x[0] if x.ndim == 1 else x[0].copy()) for k, x in table_from_arrays(counts[-1:], measures[-1:]).items()}

    @property
    def is_watertight(self):
        """Every component closed and oriented, none with a face that repeats an index (and at least one component)."""
        t = self.table
        return bool(self.n_components > 0 and t["closed_oriented"].all() and not t["degenerate"].any())


class _Run:
    """One s3d_mesh_topology_run and its workspace; keep() may follow any number of times."""

    def __init__(self, vertices, faces, weld):
        torch = _torch()
        self.device = _device_of(vertices, faces)
        self.vd = _dev(vertices, torch.float64, self.device).reshape(-1, 3)
        self.fd = _dev(faces, torch.int64, self.device).reshape(-1, 3)
        self.L, self.lib = _lib()
        self.nv, self.nf, self.weld = self.vd.shape[0], self.fd.shape[0], int(bool(weld))
        self.nb = self.lib.s3d_mesh_topology_workspace_bytes(self.nv, self.nf, self.weld)
        if self.nb == 0:
            raise ValueError("mesh_topology: %d vertices, %d faces cannot be served" % (self.nv, self.nf))
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device=self.device)
        k, rounds = C.c_long(0), C.c_int(0)
        self.L.check(self.lib.s3d_mesh_topology_run(self.vd.data_ptr(), self.nv, self.fd.data_ptr(), self.nf, self.weld,
                                                    self.ws.data_ptr(), self.nb, C.byref(k), C.byref(rounds), None, self.st),
                     "s3d_mesh_topology_run")
        self.k, self.rounds = k.value, rounds.value

    @property
    def st(self):
        """the stream current at the time of each call (run, emit and keep need not share one)"""
        return self.L.stream_ptr(self.device)

    def keep(self, mask, drop_degenerate=False):
        """-> (vertices, faces) device tensors of the components `mask` selects."""
        torch = _torch()
        mask = np.asarray(mask, dtype=bool).reshape(-1)
        if len(mask) != self.k:
            raise ValueError("keep: %d flags for %d components" % (len(mask), self.k))
        flags = torch.from_numpy(mask.astype(np.uint8)).to(self.device)
        nvo, nfo = C.c_long(0), C.c_long(0)
        self.L.check(self.lib.s3d_mesh_topology_keep_run(self.ws.data_ptr(), self.nb, self.nv, self.nf, self.weld, self.k,
                                                         flags.data_ptr(), int(bool(drop_degenerate)), C.byref(nvo),
                                                         C.byref(nfo), self.st), "s3d_mesh_topology_keep_run")
        vo = torch.empty((nvo.value, 3), dtype=torch.float64, device=self.device)
        fo = torch.empty((nfo.value, 3), dtype=torch.int64, device=self.device)
        if nvo.value and nfo.value:
            self.L.check(self.lib.s3d_mesh_topology_keep_emit(self.ws.data_ptr(), self.nb, self.vd.data_ptr(), self.nv, self.nf,
                                                              self.weld, vo.data_ptr(), fo.data_ptr(), self.st),
                         "s3d_mesh_topology_keep_emit")
        return vo, fo


def mesh_topology(mesh, weld=False):
    """Components, labels and the table of `mesh` (after welding equal positions with weld=True)."""
    v, f = _mesh_arrays(mesh)
    return MeshTopology(_Run(v, f, weld), f)


def weld(vertices, faces):
    """-> (vertices, faces, vmap): the mesh over the representatives that faces reference, in ascending original index, and
    vmap (V,) int64, the original index of every input vertex's representative.  A referenced vertex with a coordinate
    that is not finite is an error; vertices that no face references are dropped (vmap keeps them as their own)."""
    topo = mesh_topology((vertices, faces), weld=True)
    vo, fo = topo._run.keep(np.ones(topo.n_components, dtype=bool))
    return _host(vo, vertices), _host(fo, faces), topo.vmap


def _measure(table, by):
    """-> (measure per component, eligible per component)."""
    if by == "faces":
        return np.asarray(table["faces"], dtype=np.float64), np.ones(len(table["faces"]), dtype=bool)
    if by == "area":
        return np.asarray(table["area"], dtype=np.float64), np.ones(len(table["area"]), dtype=bool)
    if by == "volume":
        ok = np.asarray(table["closed_oriented"], dtype=bool)
        return np.where(ok, np.abs(np.asarray(table["volume"], dtype=np.float64)), 0.0), ok
    raise ValueError("by must be 'faces', 'area' or 'volume', got %r" % (by,))


def select_components(table, largest=None, by="faces", min_faces=0, min_frac=0.0):
    """-> bool mask (K,) of the components that pass every rule given:
      largest=n      among the n largest in the `by` measure (ties go to the lower component id);
      min_faces=n    at least n faces;
      min_frac=x     at least x times the largest component's `by` measure.
    by="volume" measures |signed volume| and requires closed_oriented: other components measure 0 and rank last."""
    m, ok = _measure(table, by)
    k = len(m)
    mask = np.ones(k, dtype=bool)
    if k == 0:
        return mask
    if min_faces:
        mask &= np.asarray(table["faces"]) >= min_faces
    if min_frac:
        mask &= ok & (m >= min_frac * m.max())
    if largest is not None:
        if largest < 0:
            raise ValueError("largest = %d < 0" % largest)
        order = np.lexsort((np.arange(k), -m, ~ok))       # eligible first, then larger first, then the lower id
        top = np.zeros(k, dtype=bool)
        top[order[:largest]] = True
        mask &= top
    return mask


def _resolve(topo, mask_or_rules):
    if isinstance(mask_or_rules, dict):
        return select_components(topo.table, **mask_or_rules)
    return np.asarray(mask_or_rules, dtype=bool).reshape(-1)


def keep_components(mesh, mask_or_rules, drop_degenerate=False, weld=False, topology=None):
    """-> Mesh of the components selected by a bool mask (K,) or by a dict of select_components' rules, faces and vertices
    in their original order.  `topology`: a MeshTopology of the same mesh and weld, to save the second run (sizes and weld are
    checked; that the arrays are the same ones is the caller's word)."""
    v, f = _mesh_arrays(mesh)
    topo = topology if topology is not None else mesh_topology((v, f), weld=weld)
    run = topo._run
    if (run.nv, run.nf, run.weld) != (len(v), len(f), int(bool(weld))):
        raise ValueError("keep_components: `topology` is of a mesh of %d vertices and %d faces with weld=%s, not of this one "
                         "(%d, %d, weld=%s)" % (run.nv, run.nf, bool(run.weld), len(v), len(f), bool(weld)))
    vo, fo = run.keep(_resolve(topo, mask_or_rules), drop_degenerate)
    return Mesh(vo.cpu().numpy(), fo.cpu().numpy())


def largest_component(mesh, by="faces"):
    return keep_components(mesh, dict(largest=1, by=by))


def split(mesh, weld=False):
    """-> one Mesh per component, in component order."""
    topo = mesh_topology(mesh, weld=weld)
    out = []
    for k in range(topo.n_components):
        vo, fo = topo._run.keep(np.arange(topo.n_components) == k)
        out.append(Mesh(vo.cpu().numpy(), fo.cpu().numpy()))
    return out
