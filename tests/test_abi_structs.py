"""CPU test of the module-tree -> C-ABI parameter-struct mapping (include/slice3d_hip.h).

Every S3d*Params struct the models and trainers hand to the library is built here from seeded CPU models, in each mode it
is used in: the eval-mode packs (`repack()` with a recording library), the training step's values and gradient slots, for
Slices3DRegModel and Slices3DGTModel.  Each pointer field is named after the tensor it points into (`grad:<name>` for a
gradient slot, None for NULL; integer fields keep their value) and compared with tests/golden/abi_struct_fields.json.
That file was recorded from the struct-building code as it stood before the builders were shared between models and
trainers, so a slot that moves, disappears or changes tensor fails here."""
import bisect
import ctypes as C
import json
import os

import pytest

from helpers import GOLDEN
from slice3d_amd.models import Slices3DRegModel, data_ptr, vgg_params
from slice3d_amd.models_gt import Slices3DGTModel
from slice3d_amd.trainer import HipGtTrainer, HipTrainer
from slice3d_amd.weights import load_seeded

GRAD_BASE = 1 << 56     # fake gradient-buffer address, above every host pointer


def _fields(struct, prefix=""):
    out = {}
    for name, typ in struct._fields_:
        val, key = getattr(struct, name), prefix + name
        if issubclass(typ, C.Structure):
            out.update(_fields(val, key + "."))
        elif issubclass(typ, C.Array) and issubclass(typ._type_, C.Structure):
            for i in range(typ._length_):
                out.update(_fields(val[i], "%s[%d]." % (key, i)))
        elif issubclass(typ, C.Array):
            out.update(("%s[%d]" % (key, i), ("ptr", val[i])) for i in range(typ._length_))
        else:
            out[key] = ("ptr" if typ is C.c_void_p else "int", val)
    return out


def _decode(struct, model, grad_names):
    spans = sorted((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), k)
                   for k, t in list(model.named_parameters()) + list(model.named_buffers()))
    starts = [lo for lo, _, _ in spans]

    def name(p):
        if p is None:
            return None
        if p >= GRAD_BASE:
            return "grad:" + grad_names[p]
        i = bisect.bisect_right(starts, p) - 1
        assert i >= 0 and p < spans[i][1], "pointer %#x is inside no parameter or buffer" % p
        return spans[i][2]
    return {k: (v if kind == "int" else name(v)) for k, (kind, v) in _fields(struct).items()}


def _trainer(cls, model):
    """A trainer of a CPU model, with fake gradient slots laid out as HipTrainer.__init__ lays out grad_flat."""
    tr = object.__new__(cls)
    tr.model, tr._gmap, grad_names, off = model, {}, {}, 0
    for k, p in model.named_parameters():
        if cls._trainable(k):
            tr._gmap[id(p)] = GRAD_BASE + 4 * off
            grad_names[GRAD_BASE + 4 * off] = k
            off += p.numel()
    return tr, grad_names


class _PackSizes:
    def __getattr__(self, symbol):
        assert symbol.endswith("_packed_bytes"), symbol
        return lambda *args: 0


def _packed_structs(model, monkeypatch):
    """The struct repack() passes to each s3d_*_pack, with the library and the device stubbed out."""
    rec = {}
    model._lib = _PackSizes()
    monkeypatch.setattr(model, "_check_packable", lambda: None)
    monkeypatch.setattr(model, "_pack", lambda symbol, params, nbytes: rec.setdefault(symbol, params))
    model.repack()
    return rec


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(GOLDEN, "abi_struct_fields.json")) as f:
        return json.load(f)


def test_reg_model_structs_match_the_recorded_mapping(want, monkeypatch):
    m = load_seeded(Slices3DRegModel(n_slices=12, backend="none"), 0)
    got = {}
    packs = _packed_structs(m, monkeypatch)
    for key, symbol in (("unet", "s3d_unet_pack"), ("head", "s3d_head_pack"), ("vgg", "s3d_vgg_pack")):
        got["pack." + key] = _decode(packs[symbol], m, {})
    tr, grad_names = _trainer(HipTrainer, m)
    (u, h), (du, dh) = tr._structs(data_ptr), tr._structs(tr._gptr)
    for key, st in (("unet", u), ("head", h), ("vgg", vgg_params(m, data_ptr)), ("unet_grad", du), ("head_grad", dh)):
        got["train." + key] = _decode(st, m, grad_names)
    for key in got:
        assert got[key] == want[key], key
    assert len(got["pack.unet"]) == 188 and len(got["pack.head"]) == 42 and len(got["pack.vgg"]) == 86


def test_gt_model_structs_match_the_recorded_mapping(want, monkeypatch):
    g = load_seeded(Slices3DGTModel(n_slices=12, backend="none"), 0)
    got = {}
    packs = _packed_structs(g, monkeypatch)
    got["gt_pack.encoder"] = _decode(packs["s3d_gt_encoder_pack"], g, {})
    got["gt_pack.head"] = _decode(packs["s3d_gt_head_pack"], g, {})
    tr, grad_names = _trainer(HipGtTrainer, g)
    (e, h), (de, dh) = tr._structs(data_ptr), tr._structs(tr._gptr)
    for key, st in (("encoder", e), ("head", h), ("encoder_grad", de), ("head_grad", dh)):
        got["gt_train." + key] = _decode(st, g, grad_names)
    for key in got:
        assert got[key] == want[key], key
