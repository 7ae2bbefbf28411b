"""UNetModel — MI355X-native counterpart of the latent-diffusion denoising U-Net
(gen_slices/ldm/modules/diffusionmodules/openaimodel.py:413-757, configured by
configs/latent-diffusion/objaverse-ldm-kl-8.yaml:22-34; BASELINE configs[4]).

Inference only.  Same constructor arguments for the options that configuration uses, the same module tree and
therefore the same state_dict keys as the reference (time_embed.*, input_blocks.N.M.{in_layers,emb_layers,
out_layers,skip_connection,norm,qkv,proj_out}.*, middle_block.*, output_blocks.*, out.*), and the same
forward(x, timesteps, c_fmaps=...) contract (NCHW in / NCHW out).  Every tensor op is an entry point of
libslice3d_hip.so, reached through the operator layer this model shares with the first stage (ldm_ops.LdmOps):
activations live channels-last, 3x3 convolutions run the LDS-staged split-precision kernel, the ResBlock residual add
and the AttentionBlock residual are conv epilogues.  There is no CPU fallback.

Not built (the configuration does not use them): class conditioning, SpatialTransformer / cross-attention,
use_new_attention_order, conv_resample down/up-sampling, fp16 torso, dims != 2.
"""
import ctypes as C
import os

import torch
import torch.nn as nn

from . import _lib
from .ldm_ops import LdmOps


def _gn(ch):
    return nn.GroupNorm(32, ch)


class ResBlock(nn.Module):
    """openaimodel.py:160-275 (use_scale_shift_norm / up / down variants)."""

    def __init__(self, channels, emb_channels, dropout, out_channels=None, use_scale_shift_norm=False, up=False,
                 down=False):
        super().__init__()
        self.channels, self.out_channels = channels, out_channels or channels
        self.use_scale_shift_norm, self.up, self.down = use_scale_shift_norm, up, down
        self.in_layers = nn.Sequential(_gn(channels), nn.SiLU(), nn.Conv2d(channels, self.out_channels, 3, padding=1))
        self.emb_layers = nn.Sequential(nn.SiLU(), nn.Linear(emb_channels, 2 * self.out_channels
                                                             if use_scale_shift_norm else self.out_channels))
        self.out_layers = nn.Sequential(_gn(self.out_channels), nn.SiLU(), nn.Dropout(p=dropout),
                                        nn.Conv2d(self.out_channels, self.out_channels, 3, padding=1))
        self.skip_connection = (nn.Identity() if self.out_channels == channels
                                else nn.Conv2d(channels, self.out_channels, 1))
        self.cat_split = None     # (C_h, C_skip) when the block's input is th.cat([h, hs.pop()]) (output blocks)


class AttentionBlock(nn.Module):
    """openaimodel.py:278-331 with QKVAttentionLegacy."""

    def __init__(self, channels, num_heads):
        super().__init__()
        self.channels, self.num_heads = channels, num_heads
        self.norm = _gn(channels)
        self.qkv = nn.Conv1d(channels, channels * 3, 1)
        self.proj_out = nn.Conv1d(channels, channels, 1)


class UNetModel(LdmOps, nn.Module):
    _NO_LIB = ("UNetModel(backend=%r) cannot compute: the HIP library is required; there is no CPU fallback in the "
               "product path")
    _NOT_EVAL = "UNetModel computes the eval-mode forward; call model.eval()"

    def __init__(self, image_size, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions,
                 dropout=0, channel_mult=(1, 2, 4, 8), num_heads=-1, use_scale_shift_norm=False, resblock_updown=False,
                 backend="hip", prec="f16x3", fuse_gn=True, branch_streams=False, defer_finish=False):
        super().__init__()
        if not resblock_updown:
            raise NotImplementedError("conv_resample down/up-sampling is not built (the Slice3D configuration uses "
                                      "resblock_updown=True)")
        if num_heads < 1:
            raise ValueError("num_heads must be set")
        self.image_size, self.in_channels, self.model_channels = image_size, in_channels, model_channels
        self.out_channels, self.num_heads = out_channels, num_heads
        # (branch_streams and defer_finish are opt-in and measured slower: see LdmOps._init_ops)
        self._init_ops(backend, prec, ("f16x3", "f16", "f32"), fuse_gn, defer_finish, branch_streams)
        ted = model_channels * 4
        self.time_embed = nn.Sequential(nn.Linear(model_channels, ted), nn.SiLU(), nn.Linear(ted, ted))
        self.input_blocks = nn.ModuleList([nn.Sequential(nn.Conv2d(in_channels, model_channels, 3, padding=1))])
        chans, ch, ds = [model_channels], model_channels, 1
        for level, mult in enumerate(channel_mult):
            for _ in range(num_res_blocks):
                layers = [ResBlock(ch, ted, dropout, mult * model_channels, use_scale_shift_norm)]
                ch = mult * model_channels
                if ds in attention_resolutions:
                    layers.append(AttentionBlock(ch, num_heads))
                self.input_blocks.append(nn.Sequential(*layers))
                chans.append(ch)
            if level != len(channel_mult) - 1:
                self.input_blocks.append(nn.Sequential(ResBlock(ch, ted, dropout, ch, use_scale_shift_norm, down=True)))
                chans.append(ch)
                ds *= 2
        self.middle_block = nn.Sequential(ResBlock(ch, ted, dropout, None, use_scale_shift_norm),
                                          AttentionBlock(ch, num_heads),
                                          ResBlock(ch, ted, dropout, None, use_scale_shift_norm))
        self.output_blocks = nn.ModuleList([])
        for level, mult in list(enumerate(channel_mult))[::-1]:
            for i in range(num_res_blocks + 1):
                ich = chans.pop()
                layers = [ResBlock(ch + ich, ted, dropout, model_channels * mult, use_scale_shift_norm)]
                layers[0].cat_split = (ch, ich)
                ch = model_channels * mult
                if ds in attention_resolutions:
                    layers.append(AttentionBlock(ch, num_heads))
                if level and i == num_res_blocks:
                    layers.append(ResBlock(ch, ted, dropout, ch, use_scale_shift_norm, up=True))
                    ds //= 2
                self.output_blocks.append(nn.Sequential(*layers))
        self.out = nn.Sequential(_gn(ch), nn.SiLU(), nn.Conv2d(model_channels, out_channels, 3, padding=1))
        # 48-wide heads at >= 1 024 tokens on the key-split f16-MFMA kernel (ldm_attn.hip la_attention2_kernel); 0 = the
        # fp32-MFMA kernel of ldm_ops.hip they ran on before round 6 (kept for the A/B)
        self.wide_head_mfma = os.environ.get("S3D_LDM_WIDE_MFMA", "1") != "0"

    # ------------------------------------------------------------------------------------------
    def _device(self):
        return self.time_embed[0].weight.device

    def _attn_precv(self):
        # prec='f16' (single-pass convolutions, the throughput mode): the attention operators keep their split-precision form
        return _lib.PREC_F32 if self.prec == "f32" else _lib.PREC_F16X3

    def repack(self):
        self._require_lib()
        if self._device().type != "cuda":
            raise _lib.S3dError("move the model to the GPU (model.cuda())")
        self._packed = {}
        for mod in self.modules():
            if isinstance(mod, ResBlock):
                # an output block's first convolution reads cat([h, skip]): packed as a two-source K loop when the fused
                # GroupNorm + convolution operator serves the block (the sources are then normalised as they are staged),
                # as one source behind the stand-alone GroupNorm otherwise (its output is one tensor)
                conv = mod.in_layers[2]
                split = mod.cat_split
                if split is not None and not (not (mod.up or mod.down) and self._gn_conv_served(
                        conv.weight.shape[0], split[0], split[1], conv.weight.shape[2])):
                    split = None
                self._pack_conv(conv, conv.weight, conv.bias, split=split)
                self._pack_conv(mod.out_layers[3], mod.out_layers[3].weight, mod.out_layers[3].bias)
                if isinstance(mod.skip_connection, nn.Conv2d):   # two-source K loop over (h, skip) for the output blocks
                    self._pack_conv(mod.skip_connection, mod.skip_connection.weight, mod.skip_connection.bias, split=mod.cat_split)
            elif isinstance(mod, AttentionBlock):
                self._pack_conv(mod.qkv, mod.qkv.weight, mod.qkv.bias)
                self._pack_conv(mod.proj_out, mod.proj_out.weight, mod.proj_out.bias)
        for conv in (self.input_blocks[0][0], self.out[2]):
            self._pack_conv(conv, conv.weight, conv.bias)
        # all ResBlock.emb_layers read the same timestep embedding: one stacked GEMV instead of one launch per block
        res = [m for m in self.modules() if isinstance(m, ResBlock)]
        self._film_w = torch.cat([m.emb_layers[1].weight for m in res], 0).contiguous()
        self._film_b = torch.cat([m.emb_layers[1].bias for m in res], 0).contiguous()
        self._film_off, off = {}, 0      # block -> first column of its (scale | shift) in the stacked output
        for m in res:
            self._film_off[m] = off
            off += m.emb_layers[1].weight.shape[0]
        self._packed_key = self._params_key()

    # ------------------------------------------------------------------------------------------
    # blocks
    # ------------------------------------------------------------------------------------------
    def _skip_branch(self, blk, xs, skip):
        """The ResBlock's 1x1 skip_connection on the side stream (forked behind everything the current stream has queued,
        i.e. behind the producers of xs / skip); returns (tensor, join) — call join() on the main stream before the tensor is
        read there.  Inside a HIP-graph capture the fork / join become graph edges: the branch runs beside the chain."""
        cur = torch.cuda.current_stream(xs.device)
        if self._side is None:
            self._side = torch.cuda.Stream(xs.device)
        side = self._side
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            res = self._conv(blk.skip_connection, xs, x1=skip, side=True)
        for t in (xs, skip):                  # allocated on the main stream, read on the side stream
            if t is not None:
                t.record_stream(side)

        def join():
            cur.wait_stream(side)
            res.record_stream(cur)            # allocated on the side stream, read on the main stream
        return res, join

    def _res_block(self, blk, x, skip=None):
        """ResBlock._forward (openaimodel.py:253-275); x (and skip: the block input is cat([x, skip]))."""
        # th.cat([h, hs.pop()], dim=1) (openaimodel.py:750) is never built: the GroupNorm reads both tensors (its groups
        # straddle them) and the 1x1 skip_connection walks them as the two sources of its K loop
        if not blk.use_scale_shift_norm:
            raise NotImplementedError("ResBlock without use_scale_shift_norm is not built")
        resampling = blk.up or blk.down
        if resampling and skip is not None:
            raise NotImplementedError("resampling ResBlock on a concatenated input (not in this architecture)")
        gn_in, conv_in, gn_out, conv_out = blk.in_layers[0], blk.in_layers[2], blk.out_layers[0], blk.out_layers[3]
        # 1. the GroupNorm of the input FIRST: if x is a deferred split-K output its statistics launch finishes it
        #    (n_in / n_out: the affine table of the fused operator where it serves the shape, the normalised tensor where not)
        fuse_in = not resampling and self._gn_conv_fusable(conv_in, x)
        n_in = self._gn_table(gn_in, x, x1=skip) if fuse_in else self._group_norm(gn_in, x, x1=skip)
        # 2. the skip path: it only needs the block's (finished) input
        xs = self._resample(x, blk.up) if resampling else x
        join = None
        if isinstance(blk.skip_connection, nn.Conv2d):
            if self.branch_streams:
                res, join = self._skip_branch(blk, xs, skip)
            else:
                res = self._conv(blk.skip_connection, xs, x1=skip)
        elif skip is not None:
            raise NotImplementedError("identity skip connection on a concatenated input (not in this architecture)")
        else:
            res = xs
        # 3. in_layers convolution (GroupNorm -> SiLU -> resample -> conv: the resampling sits between, nothing to fuse)
        if fuse_in:
            h = self._gn_conv_apply(conv_in, x, skip, n_in)
        else:
            h = self._conv(conv_in, self._resample(n_in, blk.up) if resampling else n_in)
        # 4. out_layers; FiLM (N, 2*Cout) = scale | shift: this block's columns of the stacked emb_layers output, read in place
        film = (self._film_all, self._film_off[blk])
        fuse_out = self._gn_conv_fusable(conv_out, h)
        n_out = self._gn_table(gn_out, h, film=film) if fuse_out else self._group_norm(gn_out, h, film=film)
        if join is not None:
            join()
        if fuse_out:
            return self._gn_conv_apply(conv_out, h, None, n_out, residual=res)
        return self._conv(conv_out, n_out, residual=res)

    def _attention_block(self, blk, x):
        """AttentionBlock._forward (openaimodel.py:309-315)."""
        lib = self._lib
        n, h, w, c = x.shape
        hn = self._group_norm(blk.norm, x, silu=False)
        qkv = self._conv(blk.qkv, hn)                                        # (N, H, W, 3C), heads x (q|k|v) x ch
        att = torch.empty((n, h, w, c), dtype=torch.float32, device=x.device)
        ch = c // blk.num_heads
        # long sequences of narrow heads: the f16-MFMA kernel with fp32-class logits and pre-split K / V (ldm_attn.hip)
        use_mfma = self._attn_precv() == _lib.PREC_F16X3
        ws_bytes = lib.s3d_qkv_attention_ws_bytes(n, h * w, blk.num_heads, ch) if use_mfma else 0
        if ws_bytes and h * w >= 1024 and (ch <= 32 or self.wide_head_mfma):
            ws = self._workspace("attn", ws_bytes, x.device)                 # (pre-split K / V block images)
            _lib.check(lib.s3d_qkv_attention_ws_fwd(qkv.data_ptr(), att.data_ptr(), n, h * w, blk.num_heads, ch, ws.data_ptr(),
                                                    ws_bytes, self._stream()), "s3d_qkv_attention_ws_fwd")
        else:
            _lib.check(lib.s3d_qkv_attention_fwd(qkv.data_ptr(), att.data_ptr(), n, h * w, blk.num_heads, ch, self._attn_precv(),
                                                 self._stream()), "s3d_qkv_attention_fwd")
        return self._conv(blk.proj_out, att, residual=x)

    def _run(self, seq, h, skip=None):
        for mod in seq:
            if isinstance(mod, ResBlock):
                h = self._res_block(mod, h, skip)
                skip = None
            elif isinstance(mod, AttentionBlock):
                h = self._attention_block(mod, h)
            else:   # the stem convolution
                h = self._conv(mod, h)
        return h

    def forward(self, x, timesteps=None, context=None, y=None, c_fmaps=None, **kwargs):
        """openaimodel.py:710-757: x (N, in_channels, H, W), timesteps (N,), c_fmaps {'f1'..'f5'} NCHW feature maps
        added after input blocks 0, 4, 7, 10, 12 -> (N, out_channels, H, W)."""
        lib = self._require_lib()
        self._require_eval()
        if context is not None or y is not None:
            raise NotImplementedError("cross-attention context / class labels are not built")
        self._ensure_packed()
        n = x.shape[0]
        self._pending = None
        t = self._f32(timesteps)
        t_emb = torch.empty((n, self.model_channels), dtype=torch.float32, device=t.device)
        _lib.check(lib.s3d_timestep_embedding_fwd(t.data_ptr(), t_emb.data_ptr(), n, self.model_channels,
                                                  C.c_float(10000.0), self._stream()), "s3d_timestep_embedding_fwd")
        te0, te2 = self.time_embed[0], self.time_embed[2]
        emb = self._linear(te2.weight, te2.bias, self._linear(te0.weight, te0.bias, t_emb, silu_in=False), silu_in=True)
        # emb_layers of every ResBlock (SiLU + Linear on the same emb, openaimodel.py:222-228,262) in one launch
        self._film_all = self._linear(self._film_w, self._film_b, emb, silu_in=True)
        inject = {0: "f1", 4: "f2", 7: "f3", 10: "f4", 12: "f5"}
        h = self._to_nhwc(x, self._pad16(self.in_channels))
        hs = []
        for m_id, module in enumerate(self.input_blocks):
            h = self._run(module, h)
            if c_fmaps is not None and m_id in inject:
                h = self._add_nchw(h, c_fmaps[inject[m_id]])
            hs.append(h)
        h = self._run(self.middle_block, h)
        for module in self.output_blocks:
            h = self._run(module, h, skip=hs.pop())
        o = self._conv(self.out[2], self._group_norm(self.out[0], h))           # (N, H, W, out_channels)
        self._finish_pending()                                                # (nothing is owed here: the stem of `out` is not split-K)
        return self._to_nchw(o)
