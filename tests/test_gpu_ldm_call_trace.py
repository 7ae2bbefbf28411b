"""The latent-diffusion route's calls into libslice3d_hip.so, pinned: for UNetModel, AutoencoderKL and ImageEncoderVGG16BN in
every mode that takes another path through the operator layer (slice3d_amd/ldm_ops.py), the ordered list of library calls from
construction to the end of the first forward equals tests/golden/ldm_call_trace.json, which
tests/golden/make_golden_ldm_call_trace.py recorded from the code BEFORE the operator layer was gathered into one module.  Same
symbols with the same non-pointer arguments in the same order = the same kernels, split counts and captured graph."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, ldm_inputs
from test_ldm import LDM_SMALL
from test_ldm_ae import AE_SMALL

FIXTURE = os.path.join(GOLDEN, "ldm_call_trace.json")
UNET_MODES = {"default": {}, "fuse_gn=False": dict(fuse_gn=False), "defer_finish=True": dict(defer_finish=True),
              "branch_streams=True": dict(branch_streams=True), "prec=f32": dict(prec="f32"), "prec=f16": dict(prec="f16")}
AE_CALLS = ("encode", "decode", "decode_12_tiles", "decode_one_tile")


def reduce_arg(a):
    """An argument as the trace keeps it: values that do not depend on where the allocator put a tensor."""
    from slice3d_amd import _lib
    if a is None:
        return "null"
    if isinstance(a, int):
        return a if abs(a) < 2 ** 32 else "ptr"
    if isinstance(a, (C.c_float, C.c_int, C.c_long)):
        return a.value
    if isinstance(a, C.c_void_p):
        return "stream"
    obj = getattr(a, "_obj", None)         # byref(...)
    if isinstance(obj, _lib.S3dConvPartial):
        return [obj.nsplit, obj.cout, obj.cin0, obj.cin1, obj.ks]
    assert obj is not None, a
    return "ref"


class Recorder:
    """Stands in for model._lib (the proxy of tools/ldm_layers.py): every callable of the library, queries included."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not callable(f):
            return f

        def call(*a):
            self.calls.append([name] + [reduce_arg(v) for v in a])
            return f(*a)
        return call


def _traced(model):
    from slice3d_amd.weights import load_seeded
    model = load_seeded(model, 0).cuda().eval()
    model._lib = Recorder(model._lib)      # right after construction: the first forward's repack() is in the trace
    return model, model._lib.calls


def run_cases(UNetModel, AutoencoderKL, ImageEncoderVGG16BN):
    """Yields (case, trace, output tensors) of every case, computed with the given classes."""
    x, t, cf = ldm_inputs(LDM_SMALL, 2, 7)
    x, t, cf = x.cuda(), t.cuda(), {k: v.cuda() for k, v in cf.items()}
    for mode, kw in UNET_MODES.items():
        m, calls = _traced(UNetModel(**dict(LDM_SMALL, **kw)))
        yield "unet/" + mode, calls, [m(x, t, c_fmaps=cf)]
    z = np.load(os.path.join(GOLDEN, "ldm_ae_small.npz"))
    img, lat = torch.from_numpy(z["x"]).cuda(), torch.from_numpy(z["z"]).cuda()
    for prec in ("f16x3", "f32"):
        for call in AE_CALLS:
            m, calls = _traced(AutoencoderKL(AE_SMALL, 4, prec=prec))
            if call == "encode":
                post = m.encode(img)
                out = [post.mean, post.logvar]
            elif call == "decode":
                out = [m.decode(lat)]
            elif call == "decode_12_tiles":
                out = [m.decode(lat, n_tiles=12)]
            else:
                out = [m.decode(lat[:, :, :16, :16].contiguous(), after_diffusion=False)]
            yield "ae/%s/%s" % (prec, call), calls, out
    m, calls = _traced(ImageEncoderVGG16BN())
    f = m(torch.rand((1, 3, 32, 32), generator=torch.Generator().manual_seed(3)).cuda())
    yield "cond/f16x3", calls, [f[k] for k in sorted(f)]


def load_fixture(path=FIXTURE):
    """case -> trace.  The file holds every distinct call once ("calls") and, per case, the indices of its calls in order."""
    z = json.load(open(path))
    return {case: [z["calls"][i] for i in idx] for case, idx in z["cases"].items()}


def _names(trace):
    return [c[0] for c in trace]


def test_the_fixture_reaches_every_path():
    """No case of the fixture is vacuous: the fused operator ran by default, not at all with fuse_gn=False, and with
    defer_finish=True a GroupNorm really took over a split-K finish pass."""
    want = load_fixture()
    assert set(want) == ({"unet/" + m for m in UNET_MODES} | {"ae/%s/%s" % (p, c) for p in ("f16x3", "f32") for c in AE_CALLS}
                         | {"cond/f16x3"})
    default, unfused, deferred = (want["unet/" + m] for m in ("default", "fuse_gn=False", "defer_finish=True"))
    assert {"s3d_conv_gn_fwd", "s3d_group_norm_table_fwd"} <= set(_names(default))
    assert not {"s3d_conv_gn_fwd", "s3d_group_norm_table_fwd"} & set(_names(unfused))
    assert ("s3d_group_norm_partial_fwd" in _names(deferred)
            or any(c[0] == "s3d_group_norm_table_fwd" and c[-2] != "null" for c in deferred))
    assert deferred != default


@pytest.mark.gpu
def test_library_calls_equal_the_recorded_trace():
    from slice3d_amd.ldm_autoencoder import AutoencoderKL, ImageEncoderVGG16BN
    from slice3d_amd.ldm_unet import UNetModel
    want = load_fixture()
    seen = set()
    for case, calls, _ in run_cases(UNetModel, AutoencoderKL, ImageEncoderVGG16BN):
        got = json.loads(json.dumps(calls))
        first = next((i for i, (a, b) in enumerate(zip(got, want[case])) if a != b), min(len(got), len(want[case])))
        assert got == want[case], (case, first, got[first:first + 1], want[case][first:first + 1])
        seen.add(case)
    torch.cuda.synchronize()
    assert seen == set(want)
