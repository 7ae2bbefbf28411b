"""Case tables, dispatch predicates, input generators and references for the kernel-by-kernel conformance of the latent-
diffusion U-Net's device code outside the convolution engine: ldm_ops.hip (GroupNorm, fp32-MFMA attention, resampling,
small linears, timestep embedding, add), ldm_attn.hip (f16-MFMA attention with split logits) and the layout / add kernels
at the end of conv.hip.  Nothing here touches a GPU: tests/test_ldm_ops_cases.py checks the tables on the CPU and
tests/test_gpu_ldm_ops.py runs them through the C ABI.

Every row's id starts with the kernel instantiation it is shaped to reach; the predicates below restate the launchers'
dispatch (launch_group_norm, launch_qkv_attention, launch_qkv_attention_ws with la_splits, launch_small_linear) in plain
Python, so a change of a switch point in the library makes the table test fail until the rows are reshaped.

Gates (`gate`): well-conditioned rows keep the project's bound 2e-5 * max(1, max|ref64|).  Rows flagged `ill` (the
x4-peaked attention rows, mean 1000 with std 0.1, the timestep embedding) are inputs on which fp32 arithmetic of the
reference's own operator (torch on the CPU) already misses that bound; there the gate is max(project bound, 4 * e_ref)
with e_ref the fp32 reference's error against float64 on that very input.  The factor 4 allows another summation order
(64-key blocks with rescaling, up to 8 key splits, 64 slice merges), not a worse error class.
"""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

TOL32 = 2e-5
TOL_POOL = 1e-6
REF_FACTOR = 4.0
GN_EPS = 1e-5
GN_SLICES = 64          # S3D_GN_SLICES (conv.h)


def seed_of(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31)


def err_and_scale(out, ref64):
    d = (out.double() - ref64).abs()
    e = float("nan") if bool(torch.isnan(d).any()) else float(d.max())
    return e, max(1.0, float(ref64.abs().max()))


def gate(ref64, ref32, ill, tol=TOL32):
    """-> (bound on max|out - ref64|, e_ref, scale)."""
    e_ref, scale = err_and_scale(ref32, ref64)
    bound = tol * scale
    if ill:
        bound = max(bound, REF_FACTOR * e_ref)
    return bound, e_ref, scale


# ------------------------------------------------------------------------------------------------------------------ GroupNorm
def gn_stats_floats(n, groups):
    return n * groups * GN_SLICES * 3


def launch_group_norm(n, hw, c, groups, table, partial=False):
    """The kernels launch_group_norm (ldm_ops.hip) runs for this shape, or None where it refuses the call."""
    if c % groups or c % 4 or n < 1 or hw < 1 or (table and groups > 64):
        return None
    per_thread = (hw * (c // groups) + 1023) // 1024
    if per_thread <= 8 or (per_thread <= 24 and n * groups >= 128):
        e = 2 if per_thread <= 2 else 8 if per_thread <= 8 else 24
        return "gn_fused<%d>%s" % (e, "+table" if table else "")
    if n * groups * 2 * 4 > 48 * 1024:
        return None
    if c <= 2048 and groups <= 1024:
        stats = "gn_stats_rows"
    else:
        if partial:
            return None
        stats = "gn_stats"
    return stats + ("+gn_table" if table else "+gn_apply")


# out: "y" (normalised output) or "table" (A | B of the fused-GroupNorm convolution); film: None, "dense" (N, 2C) or "wide"
# (a column range of a wider tensor: film_stride > 2C; one-tensor and table entry points); c0: channels of source 0 (0: one
# tensor); inp: generator name
GnCase = namedtuple("GnCase", "id kernel n hw c groups c0 out film silu inp ill")


def _gn(kernel, tag, n, hw, c, groups, c0, out, film, silu, inp, ill=False):
    return GnCase("%s-%s" % (kernel, tag), kernel, n, hw, c, groups, c0, out, film, silu, inp, ill)


GN_CASES = [
    # one-launch paths
    _gn("gn_fused<2>", "c96-g32", 2, 120, 96, 32, 0, "y", "dense", 1, "normal"),
    _gn("gn_fused<2>+table", "c64-g8-n3", 3, 77, 64, 8, 0, "table", "wide", 0, "mean50"),
    _gn("gn_fused<2>", "hw1-g8-n3", 3, 1, 96, 8, 0, "y", None, 0, "normal"),
    _gn("gn_fused<2>", "c4-g1-n5-const", 5, 300, 4, 1, 0, "y", "dense", 1, "const"),
    _gn("gn_fused<2>", "two-straddle", 2, 100, 96, 8, 40, "y", "dense", 1, "offsets"),
    _gn("gn_fused<8>", "c64-g8-hw1000", 2, 1000, 64, 8, 0, "y", "wide", 1, "offsets"),
    _gn("gn_fused<8>+table", "c2048-g1-hw4", 2, 4, 2048, 1, 0, "table", "dense", 0, "normal"),   # C / groups > 1024 threads
    _gn("gn_fused<8>+table", "two-straddle", 1, 600, 192, 32, 100, "table", None, 0, "mean50"),
    _gn("gn_fused<8>", "slabfirst", 1, 1024, 64, 8, 0, "y", None, 1, "slabfirst"),
    _gn("gn_fused<8>", "c2048-g64-n3", 3, 70, 2048, 64, 0, "y", "dense", 1, "images"),
    _gn("gn_fused<24>", "c192-g32-n4", 4, 4096, 192, 32, 0, "y", "dense", 1, "images"),
    _gn("gn_fused<24>+table", "c256-g64", 2, 2500, 256, 64, 0, "table", "wide", 0, "offsets"),
    _gn("gn_fused<24>", "mean1000", 4, 3000, 96, 32, 0, "y", None, 0, "mean1000", True),
    # sliced: coalesced one-pass partial moments + apply / table
    _gn("gn_stats_rows+gn_apply", "c96-hw4099", 2, 4099, 96, 32, 0, "y", "dense", 1, "normal"),
    _gn("gn_stats_rows+gn_apply", "slabfirst-c192", 1, 16384, 192, 32, 0, "y", None, 0, "slabfirst"),
    _gn("gn_stats_rows+gn_apply", "c2048-g1-hw5", 3, 5, 2048, 1, 0, "y", "wide", 1, "normal"),   # HW < 64: empty slices
    _gn("gn_stats_rows+gn_apply", "mean1000", 2, 5000, 64, 8, 0, "y", None, 0, "mean1000", True),
    _gn("gn_stats_rows+gn_apply", "two-straddle", 2, 3000, 96, 8, 40, "y", "dense", 1, "mean50"),
    _gn("gn_stats_rows+gn_apply", "c4-g1-const", 3, 9001, 4, 1, 0, "y", "dense", 1, "const"),
    _gn("gn_stats_rows+gn_apply", "c2048-g64", 1, 700, 2048, 64, 0, "y", "dense", 1, "offsets"),
    _gn("gn_stats_rows+gn_apply", "n5-g8-images", 5, 2100, 128, 8, 0, "y", None, 1, "images"),
    _gn("gn_stats_rows+gn_table", "c96-hw4099", 2, 4099, 96, 32, 0, "table", "wide", 0, "normal"),
    _gn("gn_stats_rows+gn_table", "slabfirst-c192", 1, 16384, 192, 32, 0, "table", None, 0, "slabfirst"),
    _gn("gn_stats_rows+gn_table", "two-straddle-g8", 3, 1500, 64, 8, 20, "table", "dense", 0, "mean50"),
    _gn("gn_stats_rows+gn_table", "c2048-g1-hw5", 2, 5, 2048, 1, 0, "table", None, 0, "normal"),
    # sliced: C > 2048
    _gn("gn_stats+gn_apply", "c2052-g4", 2, 40, 2052, 4, 0, "y", "dense", 1, "normal"),
    _gn("gn_stats+gn_apply", "c2052-g1-hw4", 3, 4, 2052, 1, 0, "y", None, 0, "mean50"),
    _gn("gn_stats+gn_apply", "two-straddle-slabfirst", 1, 30, 2052, 4, 1000, "y", "dense", 1, "slabfirst"),
    _gn("gn_stats+gn_table", "c2052-g36", 2, 150, 2052, 36, 0, "table", "wide", 0, "offsets"),
]
GN_KERNELS = ["gn_fused<2>", "gn_fused<8>", "gn_fused<24>", "gn_fused<2>+table", "gn_fused<8>+table", "gn_fused<24>+table",
              "gn_stats_rows+gn_apply", "gn_stats_rows+gn_table", "gn_stats+gn_apply", "gn_stats+gn_table"]

# source 0 = the raw split-K partial sums of a convolution (s3d_group_norm_partial_fwd, s3d_group_norm_table_fwd(x0_partial));
# c1: channels of a finished second source (table entry point only); nsplit 1 is refused by the descriptor check
GnPartialCase = namedtuple("GnPartialCase", "id kernel n hw c0 c1 groups out nsplit bias res film silu")


def _gp(kernel, n, hw, c0, c1, groups, out, nsplit, bias, res, film, silu):
    tag = "ns%d%s%s" % (nsplit, "-bias" if bias else "", "-res" if res else "")
    return GnPartialCase("%s-partial-%s" % (kernel, tag), kernel, n, hw, c0, c1, groups, out, nsplit, bias, res, film, silu)


GN_PARTIAL_CASES = [
    _gp("gn_fused<2>", 2, 20, 64, 0, 32, "y", 3, True, True, "dense", 1),
    _gp("gn_fused<2>", 2, 20, 64, 0, 32, "y", 4, False, False, None, 0),
    _gp("gn_fused<2>", 3, 21, 64, 0, 8, "y", 5, True, False, "wide", 1),
    _gp("gn_fused<2>", 2, 20, 64, 0, 32, "y", 9, False, True, None, 1),
    _gp("gn_fused<8>+table", 2, 600, 64, 32, 8, "table", 4, False, False, "dense", 0),
    _gp("gn_fused<24>", 4, 4200, 64, 0, 32, "y", 3, False, True, None, 1),
    _gp("gn_stats_rows+gn_apply", 1, 4100, 64, 0, 32, "y", 3, False, True, None, 1),
    _gp("gn_stats_rows+gn_apply", 1, 4100, 64, 0, 32, "y", 4, True, True, "wide", 1),
    _gp("gn_stats_rows+gn_apply", 1, 4101, 64, 0, 32, "y", 5, True, False, "dense", 0),
    _gp("gn_stats_rows+gn_apply", 1, 4100, 64, 0, 32, "y", 9, False, False, None, 0),
    _gp("gn_stats_rows+gn_apply", 1, 16500, 64, 0, 32, "y", 5, True, True, "dense", 1),    # slabs of 257 / 258 rows on 64 lanes
    _gp("gn_stats_rows+gn_table", 2, 2100, 64, 64, 32, "table", 9, True, True, "wide", 0),
    _gp("gn_stats_rows+gn_table", 2, 2100, 64, 64, 32, "table", 3, False, False, None, 0),
]
GN_PARTIAL_REFUSED = _gp("gn_fused<2>", 2, 20, 64, 0, 32, "y", 1, True, True, None, 0)


def gn_rows_loop_trips(hw, c):
    """(trips of the four-rows-in-flight loop, trips of the one-row tail loop) summed over every slab and pixel lane of
    gn_stats_rows_kernel for an (hw, c) map."""
    lanes = 1024 // (c // 4)
    main = tail = 0
    for sl in range(GN_SLICES):
        p0, p1 = hw * sl // GN_SLICES, hw * (sl + 1) // GN_SLICES
        for pr in range(lanes):
            p = p0 + pr
            while p + 3 * lanes < p1:
                main += 1
                p += 4 * lanes
            while p < p1:
                tail += 1
                p += lanes
    return main, tail


def gn_slab_starts(hw):
    return sorted({hw * sl // GN_SLICES for sl in range(GN_SLICES) if hw * (sl + 1) // GN_SLICES > hw * sl // GN_SLICES})


def gn_input(inp, n, hw, c, groups, g):
    """(N, HW, C) fp32 input of generator `inp`."""
    x = torch.randn(n, hw, c, generator=g)
    if inp == "normal":
        pass
    elif inp == "mean50":
        x = x + 50.0
    elif inp == "mean1000":
        x = x * 0.1 + 1000.0
    elif inp == "offsets":           # per-channel offsets of a few standard deviations
        x = x + 5.0 * torch.randn(c, generator=g)
    elif inp == "slabfirst":         # +300 on the first pixel of every pixel slab of the sliced statistics kernels
        x[:, gn_slab_starts(hw), :] += 300.0
    elif inp == "const":             # group 0 of image 0 constant: variance 0, the output is beta through FiLM and SiLU
        x[0, :, :c // groups] = 2.5
    elif inp == "images":            # every image with its own scale and mean
        for i in range(n):
            x[i] = x[i] * (1.0 + i) + 3.0 * i - 2.0
    else:
        raise ValueError(inp)
    return x.contiguous()


def gn_params(c, n, film, g):
    """gamma, beta, film tensor (or None), film_stride, column offset of this layer's (scale | shift) in the film tensor."""
    gamma = 1.0 + 0.3 * torch.randn(c, generator=g)
    beta = 0.3 * torch.randn(c, generator=g)
    if film is None:
        return gamma, beta, None, 0, 0
    if film == "dense":
        return gamma, beta, 0.3 * torch.randn(n, 2 * c, generator=g), 2 * c, 0
    off = 8
    return gamma, beta, 0.3 * torch.randn(n, 2 * c + 24, generator=g), 2 * c + 24, off


def gn_ref(x, groups, gamma, beta, film_cols, silu, dtype):
    """GroupNorm -> FiLM -> SiLU of (N, HW, C) in `dtype` on the CPU; film_cols = (N, 2C) scale | shift or None."""
    n, hw, c = x.shape
    y = F.group_norm(x.to(dtype).permute(0, 2, 1), groups, gamma.to(dtype), beta.to(dtype), GN_EPS)
    if film_cols is not None:
        f = film_cols.to(dtype)
        y = y * (1 + f[:, :c, None]) + f[:, c:2 * c, None]
    if silu:
        y = F.silu(y)
    return y.permute(0, 2, 1).contiguous()


# ------------------------------------------------------------------------------------------------------------------ attention
QA_WIDTHS = (8, 16, 24, 32, 48, 64, 96)


def launch_qkv_attention(n, t, heads, ch):
    if ch not in QA_WIDTHS:
        return None
    blocks = n * heads * ((t + 63) // 64)
    split = blocks <= 1024 and ch <= 48 and t > 64
    return "qkv_attention<%d,%d>" % (ch, 2 if split else 1)


def la_splits(n, t, heads):
    nblk = (t + 63) // 64
    base = n * heads * ((t + 63) // 64)
    s = 1
    while base * s < 512 and 2 * s * 2 <= nblk and s < 8:
        s *= 2
    return s


def launch_qkv_attention_ws(n, t, heads, ch):
    """-> (kernel, key splits); (None, 0) for the widths s3d_qkv_attention_ws_bytes answers with 0."""
    if ch % 8 or (ch > 32 and ch != 48):
        return None, 0
    blocks2 = n * heads * ((t + 127) // 128)
    if ch == 48:
        if blocks2 >= 512:
            return "la_attention2<48,2>", 1
        ns = la_splits(n, t, heads)
        return "la_attention2<48,1>" + ("+la_merge<48>/s%d" % ns if ns > 1 else "/s1"), ns
    return "la_attention<%d,%d>" % (ch, 2 if blocks2 >= 512 else 1), 1


WS_UNSERVED_WIDTHS = (12, 40, 64, 96)

AttnCase = namedtuple("AttnCase", "id entry kernel n t heads ch inp ill")


def _at(entry, kernel, n, t, heads, ch, inp, ill=False):
    return AttnCase("%s-T%d-n%dh%d-%s" % (kernel, t, n, heads, inp), entry, kernel, n, t, heads, ch, inp, ill)


ATTN_CASES = [
    # s3d_qkv_attention_fwd, four waves: T <= 64 for the widths that otherwise split the keys; the wide heads at any T
    _at("fwd", "qkv_attention<8,1>", 2, 1, 3, 8, "normal"),
    _at("fwd", "qkv_attention<8,1>", 1, 64, 2, 8, "falling"),
    _at("fwd", "qkv_attention<16,1>", 2, 15, 2, 16, "peaked", True),
    _at("fwd", "qkv_attention<16,1>", 4, 1025, 16, 16, "normal"),          # 1088 workgroups: above the key-split cap
    _at("fwd", "qkv_attention<24,1>", 2, 16, 3, 24, "dom_last"),
    _at("fwd", "qkv_attention<32,1>", 1, 17, 2, 32, "allequal"),
    _at("fwd", "qkv_attention<48,1>", 2, 63, 2, 48, "rising"),
    _at("fwd", "qkv_attention<64,1>", 2, 65, 2, 64, "normal"),
    _at("fwd", "qkv_attention<64,1>", 1, 193, 2, 64, "peaked", True),
    _at("fwd", "qkv_attention<96,1>", 1, 127, 2, 96, "dom_first"),
    _at("fwd", "qkv_attention<96,1>", 2, 129, 1, 96, "offset"),
    # eight waves, two key halves: even and odd counts of 64-key blocks (odd: half 1's last trip is fully masked)
    _at("fwd", "qkv_attention<8,2>", 2, 65, 2, 8, "normal"),
    _at("fwd", "qkv_attention<8,2>", 1, 129, 3, 8, "peaked", True),
    _at("fwd", "qkv_attention<16,2>", 2, 128, 2, 16, "rising"),
    _at("fwd", "qkv_attention<16,2>", 1, 129, 2, 16, "dom_last"),
    _at("fwd", "qkv_attention<24,2>", 1, 193, 2, 24, "falling"),
    _at("fwd", "qkv_attention<24,2>", 2, 129, 2, 24, "allequal"),
    _at("fwd", "qkv_attention<32,2>", 2, 127, 2, 32, "offset"),
    _at("fwd", "qkv_attention<32,2>", 1, 129, 3, 32, "dom_first"),
    _at("fwd", "qkv_attention<48,2>", 2, 65, 2, 48, "peaked", True),
    _at("fwd", "qkv_attention<48,2>", 1, 129, 2, 48, "normal"),
    _at("fwd", "qkv_attention<48,2>", 1, 1025, 2, 48, "dom_last"),         # 17 blocks, ragged last one
    # s3d_qkv_attention_ws_fwd, narrow heads, one query tile per wave
    _at("ws", "la_attention<8,1>", 2, 1, 3, 8, "normal"),
    _at("ws", "la_attention<8,1>", 1, 129, 2, 8, "rising"),
    _at("ws", "la_attention<16,1>", 2, 15, 2, 16, "peaked", True),
    _at("ws", "la_attention<16,1>", 1, 65, 3, 16, "dom_last"),
    _at("ws", "la_attention<24,1>", 2, 16, 2, 24, "allequal"),
    _at("ws", "la_attention<24,1>", 1, 193, 2, 24, "falling"),
    _at("ws", "la_attention<24,1>", 1, 1025, 4, 24, "dom_last"),
    _at("ws", "la_attention<32,1>", 2, 17, 2, 32, "offset"),
    _at("ws", "la_attention<32,1>", 1, 63, 2, 32, "normal"),
    _at("ws", "la_attention<32,1>", 2, 64, 1, 32, "dom_first"),
    _at("ws", "la_attention<32,1>", 1, 127, 2, 32, "peaked", True),
    # two query tiles per wave: N * heads * ceil(T / 128) >= 512
    _at("ws", "la_attention<8,2>", 4, 1025, 16, 8, "normal"),
    _at("ws", "la_attention<16,2>", 4, 1025, 16, 16, "dom_last"),
    _at("ws", "la_attention<24,2>", 4, 1025, 16, 24, "rising"),
    _at("ws", "la_attention<32,2>", 4, 1025, 16, 32, "peaked", True),
    # 48-wide heads: two k-steps; 1, 2, 4, 8 key splits + merge
    _at("ws", "la_attention2<48,2>", 4, 1025, 16, 48, "normal"),
    _at("ws", "la_attention2<48,1>/s1", 1, 1, 1, 48, "normal"),
    _at("ws", "la_attention2<48,1>/s1", 2, 63, 2, 48, "falling"),
    _at("ws", "la_attention2<48,1>/s1", 2, 128, 2, 48, "peaked", True),
    _at("ws", "la_attention2<48,1>+la_merge<48>/s2", 1, 257, 3, 48, "dom_last"),
    _at("ws", "la_attention2<48,1>+la_merge<48>/s2", 2, 257, 2, 48, "peaked", True),
    _at("ws", "la_attention2<48,1>+la_merge<48>/s4", 1, 513, 2, 48, "rising"),
    _at("ws", "la_attention2<48,1>+la_merge<48>/s4", 1, 1100, 8, 48, "dom_first"),
    _at("ws", "la_attention2<48,1>+la_merge<48>/s8", 1, 1025, 2, 48, "normal"),     # 17 blocks over 8 splits
    _at("ws", "la_attention2<48,1>+la_merge<48>/s8", 1, 1025, 2, 48, "offset"),
]
ATTN_KERNELS = (["qkv_attention<%d,1>" % c for c in QA_WIDTHS] + ["qkv_attention<%d,2>" % c for c in (8, 16, 24, 32, 48)]
                + ["la_attention<%d,%d>" % (c, q) for c in (8, 16, 24, 32) for q in (1, 2)]
                + ["la_attention2<48,2>", "la_attention2<48,1>/s1"]
                + ["la_attention2<48,1>+la_merge<48>/s%d" % s for s in (2, 4, 8)])
ATTN_T_VALUES = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 193)


def attn_input(inp, n, t, heads, ch, g):
    """qkv (N, T, heads, 3, ch) fp32: the token-major output of the qkv 1x1 convolution."""
    qkv = torch.randn(n, t, heads, 3, ch, generator=g)
    q, k = qkv[:, :, :, 0], qkv[:, :, :, 1]
    root = math.sqrt(ch)        # a product q0 * k0 = a * root adds a to the logit (the scale is ch^-1/4 on each side)
    if inp == "normal":
        pass
    elif inp == "peaked":        # logits x16: a few keys carry the whole softmax
        q *= 4.0
        k *= 4.0
    elif inp == "offset":        # large common part of the logits (the k offset alone is a per-query constant: softmax unchanged)
        k += 16.0
        q += 0.25
    elif inp in ("dom_first", "dom_last"):   # one key wins every query by e^12: in the first block / in the last, ragged one
        j = 3 % t if inp == "dom_first" else t - 1
        q[..., 0] = 4.0
        k[..., 0] = 0.0
        k[:, j, :, 0] = 3.0 * root
    elif inp in ("rising", "falling"):       # the running maximum moves in every block / is set by the first key
        ramp = torch.arange(t, dtype=torch.float32) * (0.0625 * root)   # + 4 per 64-key block, above the random part
        q[..., 0] = 1.0
        k[..., 0] = (ramp if inp == "rising" else -ramp)[None, :, None]
    elif inp == "allequal":      # every key the same: uniform softmax, the output is the mean of V
        k[:] = k[:, :1].clone()
    else:
        raise ValueError(inp)
    return qkv.contiguous()


def attn_ref(qkv, dtype):
    """QKVAttentionLegacy (scale ch^-1/4 on q and on k, softmax over the keys) -> (N, T, heads * ch) in `dtype`."""
    n, t, heads, _, ch = qkv.shape
    scale = 1 / math.sqrt(math.sqrt(ch))
    out = torch.empty(n, t, heads, ch, dtype=dtype)
    for i in range(n):           # image by image: (heads, T, T) weights at a time
        x = qkv[i].to(dtype)
        q, k, v = x[:, :, 0].permute(1, 0, 2), x[:, :, 1].permute(1, 0, 2), x[:, :, 2].permute(1, 0, 2)   # (heads, T, ch)
        w = torch.softmax(torch.bmm(q * scale, (k * scale).transpose(1, 2)), dim=-1)
        out[i] = torch.bmm(w, v).permute(1, 0, 2)
    return out.reshape(n, t, heads * ch)


# --------------------------------------------------------------------------------------------------------------- small layers
def launch_small_linear(n, k, m, w_aligned16=True):
    if m >= 4096 and k % 4 == 0 and 4 * k * 4 <= 48 * 1024 and w_aligned16:
        return "small_linear"
    return "small_linear_scalar"


# woff: the weight matrix is a view `woff` floats into its allocation (1: not 16-byte aligned)
LinCase = namedtuple("LinCase", "id kernel n k m silu bias woff")


def _ln(kernel, n, k, m, silu, bias, woff=0):
    return LinCase("%s-n%d-k%d-m%d%s%s%s" % (kernel, n, k, m, "-silu" if silu else "", "" if bias else "-nobias",
                                              "-woff%d" % woff if woff else ""), kernel, n, k, m, silu, bias, woff)


LIN_CASES = [
    _ln("small_linear", 1, 256, 4096, 1, True),
    _ln("small_linear_scalar", 4, 256, 4095, 1, True),
    _ln("small_linear", 5, 3072, 4096, 1, True),
    _ln("small_linear_scalar", 8, 3076, 4096, 0, True),
    _ln("small_linear_scalar", 9, 256, 4100, 1, True, 1),
    _ln("small_linear", 9, 192, 4099, 0, False),            # M % 16 != 0: the last wave pass has three rows
    _ln("small_linear", 8, 64, 4112, 1, True),
    _ln("small_linear", 4, 768, 4512 + 3, 1, False),
    _ln("small_linear", 5, 8, 131072 + 40, 0, True),         # beyond 8192 x 16 rows: the grid-stride loop
    _ln("small_linear_scalar", 1, 770, 33, 1, False),
    _ln("small_linear_scalar", 5, 5, 7, 0, True),
]
LIN_KERNELS = ("small_linear", "small_linear_scalar")


def lin_input(case, g):
    x = torch.randn(case.n, case.k, generator=g)
    w = torch.randn(case.m, case.k, generator=g) / math.sqrt(case.k)
    b = 0.5 * torch.randn(case.m, generator=g) if case.bias else None
    return x, w, b


def lin_ref(x, w, b, silu, dtype):
    xd = x.to(dtype)
    return F.linear(F.silu(xd) if silu else xd, w.to(dtype), b.to(dtype) if b is not None else None)


# (id, N, dim): t cycles through TS_VALUES
TS_VALUES = (0.0, 1.0, 0.5, 999.0)
TS_CASES = [("even320", 4, 320), ("odd321", 5, 321), ("dim2", 4, 2), ("odd3", 4, 3), ("even192-n9", 9, 192)]
TS_MAX_PERIOD = 10000.0


def ts_input(n):
    return torch.tensor([TS_VALUES[i % len(TS_VALUES)] for i in range(n)], dtype=torch.float32)


def ts_ref(t, dim, dtype):
    """timestep_embedding of the reference's util.py: [cos(t f) | sin(t f) | 0 if dim is odd], f_i = max_period^(-i / half)."""
    half = dim // 2
    freqs = torch.exp(-math.log(TS_MAX_PERIOD) * torch.arange(half, dtype=dtype) / half)
    args = t.to(dtype)[:, None] * freqs[None]
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    if dim % 2:
        emb = torch.cat([emb, torch.zeros_like(emb[:, :1])], dim=-1)
    return emb


# (id, up, N, H, W, C); *-cap: more than 4096 blocks of 256 threads' worth of float4 outputs
RESAMPLE_CASES = [
    ("up-odd-c4", 1, 2, 5, 7, 4), ("up-3x3-c64", 1, 1, 3, 3, 64), ("up-cap", 1, 1, 65, 65, 256),
    ("down-2x2-c4", 0, 2, 2, 2, 4), ("down-12x10-c96", 0, 2, 12, 10, 96), ("down-cap", 0, 1, 258, 260, 256),
]


def resample_blocks(up, n, h, w, c):
    total = n * 4 * h * w * (c // 4) if up else n * (h // 2) * (w // 2) * (c // 4)
    return (total + 255) // 256


def resample_ref(x, up, dtype):
    """x (N, H, W, C) -> nearest 2x / 2x2 average pool, channels-last."""
    xd = x.to(dtype).permute(0, 3, 1, 2)
    y = F.interpolate(xd, scale_factor=2, mode="nearest") if up else F.avg_pool2d(xd, 2)
    return y.permute(0, 2, 3, 1).contiguous()


ADD_CASES = [4, 1028, 4096 * 256 * 4 + 4]                                  # floats; the last one is above the grid cap
ADD_NCHW_CASES = [(2, 5, 3, 7), (1, 96, 12, 10), (1, 33, 260, 250)]          # (N, C, H, W)
NCHW_PAD_CASES = [(2, 3, 5, 7, 16), (1, 4, 3, 3, 4), (3, 5, 9, 4, 8), (1, 13, 400, 330, 16)]   # (N, C, H, W, cpad)


# ------------------------------------------------------------------------------------------------------------------- builders
def gn_build(case):
    """Inputs and references of a GN_CASES row: x (N, HW, C), gamma, beta, film / film_stride / film_off, ref64, ref32.
    Table rows are compared as y = x * A + B, so their reference has no SiLU."""
    g = torch.Generator().manual_seed(seed_of(case.id))
    x = gn_input(case.inp, case.n, case.hw, case.c, case.groups, g)
    gamma, beta, film, fstride, foff = gn_params(case.c, case.n, case.film, g)
    cols = film[:, foff:foff + 2 * case.c] if film is not None else None
    silu = case.silu if case.out == "y" else 0
    return dict(x=x, gamma=gamma, beta=beta, film=film, film_stride=fstride, film_off=foff,
                ref64=gn_ref(x, case.groups, gamma, beta, cols, silu, torch.float64),
                ref32=gn_ref(x, case.groups, gamma, beta, cols, silu, torch.float32))


def gn_partial_build(case):
    """A GN_PARTIAL_CASES row: parts (nsplit, N, HW, c0), bias (c0) or None, res (N, HW, c0) or None, x1 (N, HW, c1) or None."""
    g = torch.Generator().manual_seed(seed_of(case.id))
    c = case.c0 + case.c1
    parts = torch.randn(case.nsplit, case.n, case.hw, case.c0, generator=g) * 0.7 + 0.2
    bias = 0.5 * torch.randn(case.c0, generator=g) if case.bias else None
    res = torch.randn(case.n, case.hw, case.c0, generator=g) if case.res else None
    x1 = (torch.randn(case.n, case.hw, case.c1, generator=g) * 1.5 + 0.3) if case.c1 else None
    gamma, beta, film, fstride, foff = gn_params(c, case.n, case.film, g)
    cols = film[:, foff:foff + 2 * c] if film is not None else None
    fin = parts.double().sum(0)
    if bias is not None:
        fin = fin + bias.double()
    if res is not None:
        fin = fin + res.double()
    x = torch.cat([fin, x1.double()], -1) if x1 is not None else fin
    silu = case.silu if case.out == "y" else 0
    return dict(parts=parts, bias=bias, res=res, x1=x1, x=x, fin64=fin, gamma=gamma, beta=beta, film=film, film_stride=fstride,
                film_off=foff, ref64=gn_ref(x, case.groups, gamma, beta, cols, silu, torch.float64),
                ref32=gn_ref(x.float(), case.groups, gamma, beta, cols, silu, torch.float32))


def attn_build(case):
    qkv = attn_input(case.inp, case.n, case.t, case.heads, case.ch, torch.Generator().manual_seed(seed_of(case.id)))
    return dict(qkv=qkv, ref64=attn_ref(qkv, torch.float64), ref32=attn_ref(qkv, torch.float32))


def lin_build(case):
    x, w, b = lin_input(case, torch.Generator().manual_seed(seed_of(case.id)))
    return dict(x=x, w=w, b=b, ref64=lin_ref(x, w, b, case.silu, torch.float64), ref32=lin_ref(x, w, b, case.silu, torch.float32))
