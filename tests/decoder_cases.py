"""Inputs, float64 references and gates for the conformance of the three decoder layers and fc_out: attn_layer_q_kernel,
ffn_layer_f16x3_pipe_kernel<0/1>, attn_last_fused_kernel and the four-launch last layer (split precision), attn_layer_kernel,
ffn_layer_kernel and attn_last_mix_kernel (exact fp32).  Nothing here touches a GPU: tests/test_decoder_cases.py checks this
file on the CPU and tests/test_gpu_decoder_layers.py runs it through Slices3DRegModel.encode / decode_stages.

Every layer is referenced from the kernels' OWN previous output (the captured token tensor, then x0, then x1 of decode_stages), so
a row's budget is the rounding of one layer and not of the chain behind it.

References of one layer on a given fp32 token tensor (R, T, 128) and a head state dict:
  ref64      oracle/ref_cpu.transformer_layer (and fc_out) in float64
  ref32      the same in fp32
  ref_split  `layer` below in float64 with every GEMM operand replaced by its split22 value: the weights, and the activations
             entering in_proj, Q K^T, P V, out_proj, linear1 and linear2; biases, softmax and LayerNorm stay exact
split22(x) = hi + lo with hi = f16(x), lo = f16(x - hi), through torch.float16 (f16 overflow and subnormal rounding included):
what an f16x3 MFMA operand carries (csrc/f16x3.h).

Gate (`gate`): max|out - ref64| <= F * max(e32, e_split) + 2^-22 * max|ref64| with e32 = max|ref32 - ref64| and
e_split = max|ref_split - ref64| (f16x3 mode only; the fp32 mode is held to F * e32 + floor).  F = query_cases.REF_FACTOR = 4
(FACTOR, per row family).  On the `seeded` weights the bound is also capped by the project's absolute bounds (CAP); on the
stress sets only the anchored bound applies.  The right-hand side comes from the CPU references alone, never from a kernel.
An sdf row of fewer than SDF_MIN_SAMPLES numbers (one per query: B = 2, Q = 1) also counts the reference error of a fixed
CPU-side population of the same case (`sdf_population_error`); every other row keeps its own.

Weight sets (WEIGHT_SETS, `weight_set`) change the head only (fc_p, fc_s, att_decoder, fc_out); each comes with the property
that makes it a stress, asserted on the CPU (`properties`, tests/test_decoder_cases.py) on tokens the CPU oracle builds.
"""
import json
import math
import os

import numpy as np
import torch

import query_cases as Q
from helpers import GOLDEN, seeded_sd_from_shapes
from oracle import ref_cpu

F64, F32 = torch.float64, torch.float32
REF_FACTOR = Q.REF_FACTOR
FLOOR_REL = Q.FLOOR_REL
FAMILIES = ("x0", "x1", "layer2", "sdf")
FACTOR = {f: REF_FACTOR for f in FAMILIES}     # per row family; raised (to at most 16) only with a cause found in the code
CAP = {"x0": 5e-5, "x1": 5e-5, "layer2": 5e-5, "sdf": 1e-4}      # the project's existing absolute bounds (seeded weights)
F16_MAX = 65504.0                              # the f16x3 operand domain
HEAD = ("fc_p.", "fc_s.", "att_decoder.", "fc_out.")
N_LAYERS = 3
WEIGHT_SETS = ("seeded", "sharp", "offset", "shift", "small")
SHARP_GAIN = 6.0                               # q and k rows of in_proj: logits x 36
OFFSET = 40.0
SHIFT = 64.0                                   # out_proj.bias and linear2.bias only: every LayerNorm row mean > 20 std
SMALL_SCALE = 2.0 ** -8

SIZE = 16                                      # image side: the smallest (the decoder does not care)
GRID_B, GRID_Q, GRID_NS = 2, (1, 17, 250), (1, 2, 7, 8, 12)       # T = 2 (minimum), 3, 8 | 9 (the `wide` switch), 13
SECOND_B, SECOND_Q, SECOND_NS, SECOND_SETS = 9, 4000, (7, 12), ("seeded", "sharp")
ATTN_BLOCKS = 4096                             # workgroups of attn_layer_q_kernel; an item is half a group of 16 queries
SUBSET_HEAD_GROUPS, SUBSET_TAIL_STRIDE = 32, 2
REF_CHUNK = 1024                               # queries per reference pass (bounds the (R, T, 2048) hidden tensor)


# ------------------------------------------------------------------------------------------------------------------ weights
_cache = {}


def full_sd(ns):
    """The seeded reference-format state dict (what load_seeded gives a Slices3DRegModel(n_slices=ns))."""
    if ("sd", ns) not in _cache:
        shapes = {k: tuple(v) for k, v in json.load(open(os.path.join(GOLDEN, "state_dict_keys.json"))).items()}
        shapes["slices_generator.emds.weight"] = (ns, 128)
        _cache[("sd", ns)] = seeded_sd_from_shapes(shapes)
    return _cache[("sd", ns)]


def weight_set(name):
    """The fp32 head state dict (fc_p, fc_s, att_decoder, fc_out; it does not depend on n_slices) of weight set `name`."""
    if ("head", name) in _cache:
        return _cache[("head", name)]
    head = {k: v.clone() for k, v in full_sd(12).items() if k.startswith(HEAD)}
    if name == "sharp":
        for l in range(N_LAYERS):
            head["att_decoder.layers.%d.self_attn.in_proj_weight" % l][:256] *= SHARP_GAIN
    elif name == "offset":
        for k in ["fc_p.bias"] + ["att_decoder.layers.%d.%s.bias" % (l, m) for l in range(N_LAYERS)
                                  for m in ("self_attn.out_proj", "linear2")]:
            head[k] += OFFSET
    elif name == "shift":   # the large-mean LayerNorm stress on all six LayerNorms: the offset enters behind the GEMMs only (an offset
                            # on fc_p.bias reaches layer 0's LayerNorm1 through Wo Wv as a spread of about 55, whatever its size)
        for l in range(N_LAYERS):
            for m in ("self_attn.out_proj", "linear2"):
                head["att_decoder.layers.%d.%s.bias" % (l, m)] += SHIFT
    elif name == "small":
        for k in head:
            if k.startswith(("fc_p.", "fc_s.")) or ".self_attn.out_proj." in k or ".linear2." in k:
                head[k] *= SMALL_SCALE
    else:
        assert name == "seeded", name
    _cache[("head", name)] = head
    return head


def head64(name):
    if ("head64", name) not in _cache:
        _cache[("head64", name)] = {k: v.double() for k, v in weight_set(name).items()}
    return _cache[("head64", name)]


# ------------------------------------------------------------------------------------------------------------------ inputs
def queries(b, q, ns):
    return Q.uniform(b, q, 7000 + 13 * q + ns)


def feed(b, ns):
    from slice3d_amd.synth import make_feed_dict
    return make_feed_dict(b, SIZE, 1, ns, seed=40 + ns, with_slices=False)


def cpu_tokens(name, b, q, ns, sel=None):
    """The fp32 token tensor (R, ns + 1, 128) the CPU oracle builds for the case (mode 'test'): the stand-in for the kernels'
    own token tensor wherever no GPU is at hand (the weight-set properties, the gate self-check).  sel = (object, query) index
    arrays: only those queries."""
    fd = feed(b, ns)
    if ("feats", b, ns) not in _cache:
        with torch.no_grad():
            _cache[("feats", b, ns)] = ref_cpu.unet_forward(full_sd(ns), fd["img_input"], ns)[0]
    feats = _cache[("feats", b, ns)]
    head = weight_set(name)
    qry = queries(b, q, ns)
    qr = ref_cpu.rotate_queries({"qry_norot": qry}, "test")
    pts = ref_cpu.project_coord(qr, fd["trans_mat_wo_rot_tp"])
    rows = []
    for ob in range(b):
        keep = torch.arange(q) if sel is None else torch.from_numpy(sel[1][sel[0] == ob])
        if keep.numel() == 0:
            continue
        tok = ref_cpu.sample_pyramid([f[ob * ns:(ob + 1) * ns] for f in feats], pts[ob:ob + 1, keep], ns)
        fp = qr[ob, keep] @ head["fc_p.weight"].t() + head["fc_p.bias"]
        fs = tok @ head["fc_s.weight"].t() + head["fc_s.bias"]
        rows.append(torch.cat([fp.view(-1, 1, 128), fs], 1))
    return torch.cat(rows, 0)


# ------------------------------------------------------------------------------------------------------------------ the second-item case
def item_round(group, n_groups):
    """Which turn of its workgroup (0 first, 1 second) handles the two items of `group` in attn_layer_q_kernel: item i of
    2 * n_groups runs on workgroup i % blocks as that workgroup's turn i // blocks, blocks = min(2 * n_groups, 4096)."""
    blocks = min(2 * n_groups, ATTN_BLOCKS)
    return (2 * group) // blocks, (2 * group + 1) // blocks


def second_item_subset(b, q):
    """(object, query) index arrays of the real queries of the reference subset, and its groups: the first 32 groups and every
    second group with index >= 2048 (queries are independent given their tokens, so the references decode only these; every
    group >= 2048 costs the float64 references 8 s per case, half of them 4.5 s — the bit-for-bit run-to-run check of the
    GPU file covers every group)."""
    gpb = (q + 15) // 16
    groups = np.concatenate([np.arange(SUBSET_HEAD_GROUPS), np.arange(ATTN_BLOCKS // 2, b * gpb, SUBSET_TAIL_STRIDE)])
    ob, qi = [], []
    for g in groups:
        q0 = (g % gpb) * 16
        n = min(16, q - q0)
        ob.append(np.full(n, g // gpb))
        qi.append(q0 + np.arange(n))
    return np.concatenate(ob), np.concatenate(qi), groups


# ------------------------------------------------------------------------------------------------------------------ references
def split22(x):
    """x as an f16x3 operand carries it, in float64: hi + lo, hi = f16(x), lo = f16(x - hi).  Exact to 2^-21 |x| for
    2^-4 <= |x| < 65520 (below, lo is an f16 subnormal: absolute 2^-25); inf where f16(x) overflows."""
    x = x.double()
    hi = x.to(torch.float16).double()
    lo = (x - hi).to(torch.float16).double()
    return torch.where(torch.isinf(hi), hi, hi + lo)


def layer(sd, x, prefix, op=None, probe=None):
    """ref_cpu.transformer_layer (eval mode) with `op` applied to every GEMM operand (None: the identity, then the two are the
    same function).  probe: a dict that receives the LayerNorm inputs, the attention probabilities, the logit range of every
    query row and the largest magnitude among the split operands."""
    f = op if op is not None else (lambda t: t)
    r, l, d = x.shape
    hd = d // ref_cpu.N_HEADS
    w = lambda k: sd[prefix + "." + k]
    qkv = f(x) @ f(w("self_attn.in_proj_weight")).t() + w("self_attn.in_proj_bias")
    q, k, v = [t.view(r, l, ref_cpu.N_HEADS, hd).transpose(1, 2) for t in qkv.split(d, dim=-1)]
    logits = (f(q) @ f(k).transpose(-1, -2)) / math.sqrt(hd)
    att = torch.softmax(logits, dim=-1)
    o = (f(att) @ f(v)).transpose(1, 2).reshape(r, l, d)
    u1 = x + (f(o) @ f(w("self_attn.out_proj.weight")).t() + w("self_attn.out_proj.bias"))
    x1 = ref_cpu.layer_norm(u1, w("norm1.weight"), w("norm1.bias"))
    hdn = torch.relu(f(x1) @ f(w("linear1.weight")).t() + w("linear1.bias"))
    u2 = x1 + (f(hdn) @ f(w("linear2.weight")).t() + w("linear2.bias"))
    out = ref_cpu.layer_norm(u2, w("norm2.weight"), w("norm2.bias"))
    if probe is not None:
        ops = [x, q, k, att, v, o, x1, hdn] + [w(n) for n in ("self_attn.in_proj_weight", "self_attn.out_proj.weight",
                                                               "linear1.weight", "linear2.weight")]
        probe.update(ln1_in=u1, ln2_in=u2, att=att, logit_range=logits.amax(-1) - logits.amin(-1),
                     operand_max=max(float(t.abs().max()) for t in ops),
                     finite=all(bool(torch.isfinite(t).all()) for t in ops + [u1, u2, out]))
    return out


def absorbed_last_tok0(sd, x, prefix):
    """Token 0 of the last layer's attention block BEFORE LayerNorm1, in the absorbed form the kernels run (decode.h): per head
    qt_h = M_h x_0 + m_h with M_h = Wk_h^T Wq_h, m_h = Wk_h^T bq_h; p = softmax_t(qt_h . x_t / sqrt(32)) (the key bias adds the
    same number to every score of a row); u = x_0 + sum_h N_h (sum_t p_t x_t) + (Wo bv + bo) with N_h = Wo[:, h] Wv_h."""
    d, nh = ref_cpu.D_MODEL, ref_cpu.N_HEADS
    hd = d // nh
    wi, bi = sd[prefix + ".self_attn.in_proj_weight"], sd[prefix + ".self_attn.in_proj_bias"]
    wo, bo = sd[prefix + ".self_attn.out_proj.weight"], sd[prefix + ".self_attn.out_proj.bias"]
    wq, wk, wv = wi[:d], wi[d:2 * d], wi[2 * d:]
    u = x[:, 0] + bo + bi[2 * d:] @ wo.t()
    for h in range(nh):
        s = slice(h * hd, (h + 1) * hd)
        m_mat, m_vec = wk[s].t() @ wq[s], wk[s].t() @ bi[:d][s]
        n_mat = wo[:, s] @ wv[s]
        qt = x[:, 0] @ m_mat.t() + m_vec
        p = torch.softmax(torch.einsum("rc,rtc->rt", qt, x) / math.sqrt(hd), dim=-1)
        u = u + torch.einsum("rt,rtc->rc", p, x) @ n_mat.t()
    return u


def _chunks(x):
    return [x[i:i + REF_CHUNK] for i in range(0, x.shape[0], REF_CHUNK)]


def layer_refs(name, x, l, prec):
    """(ref64, ref32, ref_split or None) of layer l on the fp32 token tensor x (R, T, 128) with weight set `name`."""
    p = "att_decoder.layers.%d" % l
    h32, h64 = weight_set(name), head64(name)
    r64 = torch.cat([ref_cpu.transformer_layer(h64, c.double(), p) for c in _chunks(x)])
    r32 = torch.cat([ref_cpu.transformer_layer(h32, c, p) for c in _chunks(x)])
    rs = torch.cat([layer(h64, c.double(), p, split22) for c in _chunks(x)]) if prec == "f16x3" else None
    return r64, r32, rs


def final_refs(name, x, prec):
    """{'layer2': (ref64, ref32, ref_split), 'sdf': (...)}: token 0 of the last layer on x (R, T, 128), then fc_out (exact in
    all three).  The split reference runs the STANDARD layer on split operands; the kernels run the absorbed form, whose
    products M = Wk^T Wq and N = Wo Wv are formed at pack time (double accumulation, rounded to fp32) and then split: an
    approximation of that layer's operand set (x_0, q~, x-bar, M, N instead of q, k, v, p, o and the four weights)."""
    lay = layer_refs(name, x, N_LAYERS - 1, prec)
    out = {"layer2": tuple(None if t is None else t[:, 0] for t in lay)}
    h32, h64 = weight_set(name), head64(name)
    fc = lambda t, h: None if t is None else (t @ h["fc_out.0.weight"].t() + h["fc_out.0.bias"]).squeeze(-1)
    t64, t32, ts = out["layer2"]
    out["sdf"] = (fc(t64, h64), fc(t32, h32), fc(ts, h64))
    return out


# ------------------------------------------------------------------------------------------------------------------ gate
def ref_error(refs):
    """e_ref = max(e32, e_split) of refs = (ref64, ref32, ref_split or None)."""
    r64, r32, rs = refs
    e_ref = float((r32.double() - r64).abs().max())
    return e_ref if rs is None else max(e_ref, float((rs - r64).abs().max()))


SDF_MIN_SAMPLES = 32
POP_Q = 250


def sdf_population_error(name, ns, prec):
    """ref_error of the sdf family on a fixed CPU-side population of the case (weight set, n_slices, prec): the 500 queries of
    the Q = 250 grid case on tokens the CPU oracle builds, taken through layers 0 and 1 by the fp32 oracle, then the last layer
    and fc_out in float64 / fp32 / split.  No kernel output enters."""
    if ("pop", name, ns, prec) not in _cache:
        x = cpu_tokens(name, GRID_B, POP_Q, ns)
        for l in range(N_LAYERS - 1):
            x = torch.cat([ref_cpu.transformer_layer(weight_set(name), c, "att_decoder.layers.%d" % l) for c in _chunks(x)])
        _cache[("pop", name, ns, prec)] = ref_error(final_refs(name, x, prec)["sdf"])
    return _cache[("pop", name, ns, prec)]


def gate(refs, family, name, ns=None, prec=None):
    """refs = (ref64, ref32, ref_split or None) -> (bound on max|out - ref64|, e_ref = max(e32, e_split)).
    sdf is ONE number per query: at B = 2, Q = 1 the row's own reference error is the larger of two numbers, which is no
    estimate of the references' error (measured 5.9e-8 on `sharp`, n_slices 2, fp32, where the layer2 row the two numbers are a
    dot product of has e_ref 1.8e-6 and the kernels sit at 1.5e-6).  An sdf row of fewer than SDF_MIN_SAMPLES numbers therefore
    takes the larger of its own reference error and sdf_population_error(name, ns, prec); every other row (Q = 17: 34 numbers,
    Q = 250, the second-item case, every row of 128 channels) is held to its own."""
    r64 = refs[0]
    e_ref = ref_error(refs)
    if family == "sdf" and r64.numel() < SDF_MIN_SAMPLES:
        e_ref = max(e_ref, sdf_population_error(name, ns, prec))
    bound = FACTOR[family] * e_ref + FLOOR_REL * float(r64.abs().max())
    return (min(bound, CAP[family]) if name == "seeded" else bound), e_ref


err = Q.err


# ------------------------------------------------------------------------------------------------------------------ properties
def properties(name, x, dtype):
    """The three layers chained in `dtype` on the token tensor x with weight set `name`: per layer the probe of `layer`."""
    head = head64(name) if dtype == F64 else weight_set(name)
    probes, h = [], x.to(dtype)
    for l in range(N_LAYERS):
        probes.append({})
        h = layer(head, h, "att_decoder.layers.%d" % l, None, probes[-1])
    return probes, h


def row_mean_over_std(u):
    return (u.mean(-1).abs() / u.std(-1, unbiased=False)).min()
