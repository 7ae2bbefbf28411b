"""LdmOps — the channels-last operator layer under the latent-diffusion route's three models (ldm_unet.UNetModel,
ldm_autoencoder.AutoencoderKL and ImageEncoderVGG16BN).  Every method is one entry point of libslice3d_hip.so
("Latent-diffusion denoising U-Net primitives" in include/slice3d_hip.h) on (N, H, W, C) fp32 tensors; all calls go through
`self._lib`.  The state, created by _init_ops() and nowhere else:

    _lib, backend, prec, _precs     the library handle (None without it), the precision name and the names the model accepts
    fuse_gn                         GroupNorm -> SiLU -> conv3x3 as one operator where the kernel serves the shape (s3d_conv_gn_fwd)
    _packed, _packed_key            key -> Packed weight image; key = the module, or (module, "qkv") / (module, "padded") for
                                    weights derived from it; the parameter versions the images were packed from
    _ws                             HipModel._workspace's dict: "splitk" / "splitk_side" (split-K scratch of the main chain / of
                                    the side stream), "attn", and whatever the model adds
    defer_finish, _pending          the split-K finish pass left to the next GroupNorm, and the one output that still owes it
    branch_streams, _side           the U-Net's skip convolutions on a side stream, and that stream
"""
import collections
import ctypes as C

import torch

from . import _lib
from .models import HipModel

Packed = collections.namedtuple("Packed", "buf cout cin0 cin1 ks")
_SPLITK_BYTES = {False: 4 * (8 << 20), True: 4 * (2 << 20)}    # main chain / side stream: they steer the library's split counts


def _ptr(t):
    return t.data_ptr() if t is not None else None


class LdmOps(HipModel):
    _BAD_PREC = None    # text of the ValueError a model raises at construction for a precision outside `precs` (None: at first use)

    def _init_ops(self, backend, prec, precs, fuse_gn=True, defer_finish=False, branch_streams=False):
        if self._BAD_PREC and prec not in precs:
            raise ValueError(self._BAD_PREC)
        self.backend, self.prec, self._precs, self.fuse_gn = backend, prec, precs, fuse_gn
        self._lib = _lib.load() if backend == "hip" else None
        self._packed, self._packed_key, self._ws = {}, None, {}
        # defer_finish: a fused-GroupNorm 3x3 convolution that ran split-K leaves its raw partial sums to the NEXT GroupNorm's
        # statistics kernel, which adds them up (+ bias + residual), stores the finished tensor and goes on with the values:
        # the convolution's own finish pass (one ~5 us launch behind ~60 of the step's 70 3x3 convolutions) is gone.  OFF by
        # default: bit-identical and measured 0.6 % SLOWER (4.203 against 4.179 ms per step, tools/ldm_ab.py,
        # profiles/r05_ldm_experiments.md) — the statistics kernels, latency-bound themselves, pay for the 5-14 partials per
        # element what the finish launches cost
        self.defer_finish = defer_finish
        self._pending = None      # (tensor, S3dConvPartial, (n, h, w), keep-alive refs) of the one deferred output, or None
        # branch_streams: a U-Net ResBlock's 1x1 skip_connection does not depend on its GroupNorm -> conv chain and runs on a
        # side stream (a parallel branch of the captured HIP graph) beside the chain's small kernels (openaimodel.py:240-246,
        # :272-275).  OFF by default: measured SLOWER on MI355X — 4.45 against 4.18 ms per step at batch 1, with runs of 7-8 ms
        # (tools/ldm_ab.py, profiles/r05_ldm_experiments.md): the graph's cross-branch dependencies cost more than the 17
        # overlapped 14 us kernels return
        self.branch_streams, self._side = branch_streams, None

    def _precv(self):
        return _lib.prec_code(self.prec, self._precs)

    def _params_key(self):
        # fuse_gn / prec decide the two-source packing of the U-Net's output blocks: toggling either after a repack() must repack
        return (self.fuse_gn, self.prec) + HipModel._params_key(self)

    @staticmethod
    def _pad16(c):
        return (c + 15) // 16 * 16

    def _pack_conv(self, key, weight, bias, split=None):
        """self._packed[key] = the packed image of a Conv2d / Conv1d(k=1) weight; split = (cin0, cin1) for two sources."""
        lib = self._lib
        cout, cin = weight.shape[0], weight.shape[1]
        ks = weight.shape[2] if weight.dim() == 4 else 1
        cin0, cin1 = split if split else (cin, 0)
        nb = lib.s3d_conv_packed_bytes(cout, cin0, cin1, ks)
        buf = torch.empty(nb, dtype=torch.uint8, device=weight.device)
        _lib.check(lib.s3d_conv_pack(weight.data_ptr(), _ptr(bias), cout, cin0, cin1, ks, buf.data_ptr(), nb, self._stream()),
                   "s3d_conv_pack")
        self._packed[key] = Packed(buf, cout, cin0, cin1, ks)

    # -- deferred split-K finish ------------------------------------------------------------------------
    def _take_pending(self, x):
        """The S3dConvPartial of x if x is the tensor whose finish pass is still owed (and hand the duty to the caller)."""
        p = self._pending
        if p is not None and p[0] is x:
            self._pending = None
            return p
        return None

    def _finish_pending(self):
        """Run the owed finish pass on its own (a consumer that is not a GroupNorm comes first, or the workspace is needed)."""
        p = self._pending
        if p is not None:
            self._pending = None
            _, desc, (n, h, w), _ = p
            _lib.check(self._lib.s3d_conv_finish_fwd(C.byref(desc), n, h, w, self._stream()), "s3d_conv_finish_fwd")

    # -- convolutions -----------------------------------------------------------------------------------
    def _conv(self, key, x0, x1=None, residual=None, side=False):
        """side: the launch is on the side stream and must not share the main chain's split-K scratch."""
        self._finish_pending()
        buf, cout, cin0, cin1, ks = self._packed[key]
        n, h, w, _ = x0.shape
        out = torch.empty((n, h, w, cout), dtype=torch.float32, device=x0.device)
        ws = self._workspace("splitk_side" if side else "splitk", _SPLITK_BYTES[side], x0.device)
        _lib.check(self._lib.s3d_conv_fwd(buf.data_ptr(), x0.data_ptr(), _ptr(x1), _ptr(residual), out.data_ptr(), n, h, w, cout,
                                          cin0, cin1, ks, self._precv(), ws.data_ptr(), _SPLITK_BYTES[side], self._stream()),
                   "s3d_conv_fwd")
        return out

    def _conv_strided(self, key, x, ho, wo, stride, pad):
        buf, cout, cin, _, ks = self._packed[key]
        n, h, w, _ = x.shape
        out = torch.empty((n, ho, wo, cout), dtype=torch.float32, device=x.device)
        _lib.check(self._lib.s3d_conv_strided_fwd(buf.data_ptr(), x.data_ptr(), out.data_ptr(), n, h, w, ho, wo, cout, cin, ks,
                                                  stride, pad, self._precv(), self._stream()), "s3d_conv_strided_fwd")
        return out

    def _gn_conv_served(self, cout, cin0, cin1, ks, h=0, w=0):
        """The C side's own statement of what s3d_conv_gn_fwd serves (s3d_conv_gn_supported) — the one source of both the
        two-source packing decision of UNetModel.repack() and the fused / unfused choice of the forward."""
        return bool(self.fuse_gn and self.prec != "f32" and
                    self._lib.s3d_conv_gn_supported(cout, cin0, cin1, ks, self._precv(), h, w, 1))

    def _gn_conv_fusable(self, key, x):
        """GroupNorm -> [FiLM] -> SiLU -> conv3x3 as one operator (s3d_conv_gn_fwd)."""
        _, cout, cin0, cin1, ks = self._packed[key]
        return (self._gn_conv_served(cout, cin0, cin1, ks, x.shape[1], x.shape[2])
                and x.shape[-1] == cin0)   # (a concatenated input needs the two-source pack)

    @staticmethod
    def _film_arg(film):
        """(pointer, row pitch) of film = (stacked (N, M) scale | shift tensor, first column), or of None."""
        return (film[0].data_ptr() + 4 * film[1], film[0].shape[1]) if film is not None else (None, 0)

    def _gn_table(self, gn, x, x1=None, film=None):
        """Statistics of group_norm(cat([x, x1])) folded with gamma / beta / FiLM into the per-channel affine table a fused
        convolution applies (s3d_group_norm_table_fwd).  If x is the deferred output of a split-K convolution this launch is
        also its finish pass (it sums the partials, adds bias and residual and stores x)."""
        lib = self._lib
        n, h, w, c = x.shape
        c1 = x1.shape[-1] if x1 is not None else 0
        stats = torch.empty(lib.s3d_group_norm_stats_floats(n, gn.num_groups), dtype=torch.float32, device=x.device)
        table = torch.empty((n, 2, c + c1), dtype=torch.float32, device=x.device)
        fp, fld = self._film_arg(film)
        pend = self._take_pending(x)
        if pend is None:
            self._finish_pending()
        _lib.check(lib.s3d_group_norm_table_fwd(x.data_ptr(), c, _ptr(x1), c1, gn.weight.data_ptr(), gn.bias.data_ptr(), fp, fld,
                                                table.data_ptr(), stats.data_ptr(), n, h * w, gn.num_groups, C.c_float(gn.eps),
                                                C.byref(pend[1]) if pend is not None else None, self._stream()),
                   "s3d_group_norm_table_fwd")
        return table

    def _gn_conv_apply(self, key, x, x1, table, residual=None):
        """conv(silu(x * A + B)) (+ residual) with the table of _gn_table: the normalised tensor is never written
        (s3d_conv_gn_fwd; openaimodel.py:188-194, :229-236, :262-270).  With defer_finish a split-K launch leaves its finish
        pass to the next consumer (self._pending)."""
        buf, cout, cin0, cin1, ks = self._packed[key]
        n, h, w, c = x.shape
        c1 = x1.shape[-1] if x1 is not None else 0
        if (c, c1) != (cin0, cin1):
            raise _lib.S3dError("fused GroupNorm convolution: sources (%d, %d) do not match the packed split (%d, %d)" % (c, c1, cin0, cin1))
        self._finish_pending()           # (the split-K scratch is about to be overwritten)
        out = torch.empty((n, h, w, cout), dtype=torch.float32, device=x.device)
        ws = self._workspace("splitk", _SPLITK_BYTES[False], x.device)
        nsplit = C.c_int(1)
        _lib.check(self._lib.s3d_conv_gn_fwd(buf.data_ptr(), x.data_ptr(), _ptr(x1), _ptr(residual), out.data_ptr(), n, h, w, cout,
                                             cin0, cin1, ks, self._precv(), table.data_ptr(), 1, ws.data_ptr(), _SPLITK_BYTES[False],
                                             C.byref(nsplit) if self.defer_finish else None, self._stream()), "s3d_conv_gn_fwd")
        if nsplit.value > 1:             # `out` is still to be written: by the next GroupNorm, or by _finish_pending()
            desc = _lib.S3dConvPartial(ws.data_ptr(), nsplit.value, buf.data_ptr(), cout, cin0, cin1, ks, _ptr(residual),
                                       out.data_ptr())
            self._pending = (out, desc, (n, h, w), (residual, buf))
        return out

    def _gn_conv(self, gn, conv_key, x, residual=None):
        """conv(swish(GroupNorm(x))) (+ residual): one fused operator where s3d_conv_gn_fwd serves the shape, else two."""
        if self._gn_conv_fusable(conv_key, x):
            return self._gn_conv_apply(conv_key, x, None, self._gn_table(gn, x), residual=residual)
        return self._conv(conv_key, self._group_norm(gn, x), residual=residual)

    def _group_norm(self, gn, x, film=None, silu=True, x1=None):
        """GroupNorm(+FiLM)(+SiLU) of x, or (without FiLM) of the channel concatenation [x, x1] (never materialised)."""
        lib = self._lib
        n, h, w, c = x.shape
        stats = torch.empty(lib.s3d_group_norm_stats_floats(n, gn.num_groups), dtype=torch.float32, device=x.device)
        rest = (gn.num_groups, C.c_float(gn.eps), 1 if silu else 0, self._stream())
        fp, fld = self._film_arg(film)
        if x1 is not None:
            if film is not None:
                raise NotImplementedError("FiLM on a two-source GroupNorm")
            self._finish_pending()
            c1 = x1.shape[-1]
            y = torch.empty((n, h, w, c + c1), dtype=torch.float32, device=x.device)
            _lib.check(lib.s3d_group_norm2_fwd(x.data_ptr(), c, x1.data_ptr(), c1, gn.weight.data_ptr(), gn.bias.data_ptr(), None,
                                               y.data_ptr(), stats.data_ptr(), n, h * w, *rest), "s3d_group_norm2_fwd")
            return y
        y = torch.empty_like(x)
        pend = self._take_pending(x)
        if pend is not None:             # x's split-K partials: the statistics kernel of this GroupNorm is its finish pass
            _lib.check(lib.s3d_group_norm_partial_fwd(C.byref(pend[1]), gn.weight.data_ptr(), gn.bias.data_ptr(), fp, fld,
                                                      y.data_ptr(), stats.data_ptr(), n, h * w, *rest), "s3d_group_norm_partial_fwd")
            return y
        self._finish_pending()
        if film is not None:
            _lib.check(lib.s3d_group_norm_film_fwd(x.data_ptr(), gn.weight.data_ptr(), gn.bias.data_ptr(), fp, fld, y.data_ptr(),
                                                   stats.data_ptr(), n, h * w, c, *rest), "s3d_group_norm_film_fwd")
        else:
            _lib.check(lib.s3d_group_norm_fwd(x.data_ptr(), gn.weight.data_ptr(), gn.bias.data_ptr(), None, y.data_ptr(),
                                              stats.data_ptr(), n, h * w, c, *rest), "s3d_group_norm_fwd")
        return y

    # -- glue -------------------------------------------------------------------------------------------
    def _resample(self, x, up):
        self._finish_pending()
        n, h, w, c = x.shape
        y = torch.empty((n, h * 2, w * 2, c) if up else (n, h // 2, w // 2, c), dtype=torch.float32, device=x.device)
        _lib.check(self._lib.s3d_resample2x_fwd(x.data_ptr(), y.data_ptr(), n, h, w, c, 1 if up else 0, self._stream()),
                   "s3d_resample2x_fwd")
        return y

    def _linear(self, weight, bias, x, silu_in):
        n, k = x.shape
        m = weight.shape[0]
        out = torch.empty((n, m), dtype=torch.float32, device=x.device)
        _lib.check(self._lib.s3d_small_linear_fwd(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), out.data_ptr(), n, k, m,
                                                  1 if silu_in else 0, self._stream()), "s3d_small_linear_fwd")
        return out

    def _add(self, a, b):
        self._finish_pending()
        out = torch.empty_like(a)
        _lib.check(self._lib.s3d_add_fwd(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), self._stream()), "s3d_add_fwd")
        return out

    def _add_nchw(self, a, b):
        """a + b with b (a U-Net c_fmap, openaimodel.py:735-746) read in the reference's NCHW layout: one launch."""
        self._finish_pending()
        b = self._f32(b)
        n, c, h, w = b.shape
        if tuple(a.shape) != (n, h, w, c):
            return self._add(a, self._to_nhwc(b))
        out = torch.empty_like(a)
        _lib.check(self._lib.s3d_add_nchw_fwd(a.data_ptr(), b.data_ptr(), out.data_ptr(), n, c, h, w, self._stream()), "s3d_add_nchw_fwd")
        return out

    def _to_nhwc(self, x, cpad=None):
        x = self._f32(x)
        n, c, h, w = x.shape
        cpad = cpad or c
        out = torch.empty((n, h, w, cpad), dtype=torch.float32, device=x.device)
        _lib.check(self._lib.s3d_nchw_to_nhwc_pad(x.data_ptr(), out.data_ptr(), n, c, h, w, cpad, self._stream()),
                   "s3d_nchw_to_nhwc_pad")
        return out

    def _to_nchw(self, x, c=None):
        """(N, C, H, W) copy of x; c: only its first c channels (a view: the padded ones stay behind)."""
        n, h, w, cs = x.shape
        out = torch.empty((n, cs, h, w), dtype=torch.float32, device=x.device)
        _lib.check(self._lib.s3d_nhwc_to_nchw(x.data_ptr(), out.data_ptr(), n, cs, h, w, self._stream()), "s3d_nhwc_to_nchw")
        return out[:, :c] if c is not None else out
