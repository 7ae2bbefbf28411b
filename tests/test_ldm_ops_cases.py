"""The case tables of tests/ldm_ops_cases.py, checked without a GPU: every row's restated dispatch predicate lands on the
kernel instantiation in its id, every instantiation has a row, the fp32 CPU reference alone meets the row's gate (so a
row's bound is attainable in fp32 arithmetic, and the rows that are not flagged ill-conditioned really are well
conditioned), and no float64 reference is slow enough to dominate the GPU run."""
import time

import pytest
import torch

import ldm_ops_cases as K

REF_SECONDS = 8.0      # per row, float64 + fp32 reference together (the largest rows take about a second)


def _ids(cases):
    return [c.id for c in cases]


def test_ids_are_unique():
    for cases in (K.GN_CASES, K.GN_PARTIAL_CASES, K.ATTN_CASES, K.LIN_CASES):
        assert len(set(_ids(cases))) == len(cases)


@pytest.mark.parametrize("case", K.GN_CASES + K.GN_PARTIAL_CASES, ids=_ids(K.GN_CASES + K.GN_PARTIAL_CASES))
def test_group_norm_rows_reach_the_kernel_in_their_id(case):
    partial = isinstance(case, K.GnPartialCase)
    c = case.c0 + case.c1 if partial else case.c
    assert K.launch_group_norm(case.n, case.hw, c, case.groups, case.out == "table", partial) == case.kernel
    assert case.id.startswith(case.kernel)
    c0 = case.c0 if case.c0 else c
    assert c0 % 4 == 0 and (c - c0) % 4 == 0 and 4 <= c0 <= c
    assert case.n * case.groups * 2 * 4 <= 48 * 1024


def test_group_norm_tables_cover_the_listed_paths_and_edges():
    rows = K.GN_CASES
    assert {c.kernel for c in rows} == set(K.GN_KERNELS)
    assert {c.kernel for c in K.GN_PARTIAL_CASES} >= {"gn_fused<2>", "gn_fused<8>+table", "gn_stats_rows+gn_apply",
                                                      "gn_stats_rows+gn_table"}
    assert {c.nsplit for c in K.GN_PARTIAL_CASES} == {3, 4, 5, 9} and K.GN_PARTIAL_REFUSED.nsplit == 1
    for kernel in ("gn_fused<2>", "gn_stats_rows+gn_apply"):     # scalar and 16-byte forms of the partial sum, with its tail
        assert {c.nsplit for c in K.GN_PARTIAL_CASES if c.kernel == kernel} == {3, 4, 5, 9}
    assert {(c.bias, c.res) for c in K.GN_PARTIAL_CASES} == {(True, True), (True, False), (False, True), (False, False)}
    assert {c.groups for c in rows} >= {1, 8, 32, 64}
    assert {c.c for c in rows} >= {4, 96, 2048, 2052}
    assert {c.film for c in rows} == {None, "dense", "wide"} and {c.silu for c in rows if c.out == "y"} == {0, 1}
    assert {c.inp for c in rows} == {"normal", "mean50", "mean1000", "offsets", "slabfirst", "const", "images"}
    assert any(c.n * c.groups % 32 for c in rows)
    assert any(c.hw == 1 for c in rows)
    sliced = [c for c in rows if c.kernel.startswith("gn_stats")]
    assert any(c.hw < K.GN_SLICES and c.kernel.startswith("gn_stats_rows") for c in sliced)        # empty slices
    assert any(c.hw % 64 for c in sliced)
    assert any(c.hw % (1024 // (c.c // 4)) for c in sliced if c.c <= 2048)                         # ragged pixel lanes
    # gn_stats_rows_kernel: the four-rows-in-flight loop and its one-row tail both run, on finished tensors and on partial sums
    for table in (rows, K.GN_PARTIAL_CASES):
        trips = [K.gn_rows_loop_trips(c.hw, c.c if table is rows else c.c0 + c.c1) for c in table
                 if c.kernel.startswith("gn_stats_rows")]
        assert any(m > 0 and t > 0 for m, t in trips), trips
        assert any(m == 0 and t > 0 for m, t in trips), trips
    assert any(c.inp == "slabfirst" and c.kernel.startswith("gn_stats_rows") for c in sliced)
    for c in rows:      # a second source puts a group across the join
        if c.c0:
            assert c.c0 % (c.c // c.groups) != 0, c.id
    assert {c.kernel for c in rows if c.c0} >= {"gn_fused<2>", "gn_fused<8>+table", "gn_stats_rows+gn_apply",
                                                 "gn_stats_rows+gn_table", "gn_stats+gn_apply"}
    assert any(c.c == 2048 and c.groups == 1 and c.hw == 4 and c.out == "table" for c in rows)    # table rows beyond 1024 threads


@pytest.mark.parametrize("case", K.ATTN_CASES, ids=_ids(K.ATTN_CASES))
def test_attention_rows_reach_the_kernel_in_their_id(case):
    if case.entry == "fwd":
        assert K.launch_qkv_attention(case.n, case.t, case.heads, case.ch) == case.kernel
    else:
        kernel, ns = K.launch_qkv_attention_ws(case.n, case.t, case.heads, case.ch)
        assert kernel == case.kernel
        assert ns == (int(case.kernel.rsplit("/s", 1)[1]) if "/s" in case.kernel else 1)
    assert case.id.startswith(case.kernel)


def test_attention_table_covers_the_listed_kernels_and_edges():
    rows = K.ATTN_CASES
    assert {c.kernel for c in rows} == set(K.ATTN_KERNELS)
    assert {c.t for c in rows} >= set(K.ATTN_T_VALUES)
    assert {c.inp for c in rows} == {"normal", "peaked", "offset", "dom_first", "dom_last", "rising", "falling", "allequal"}
    assert all(c.ill == (c.inp == "peaked") for c in rows)      # only the x4-peaked rows take the reference-relative gate
    for ch in (8, 16, 24, 32, 48):      # both parities of the 64-key block count on the two-half kernel
        par = {((c.t + 63) // 64) % 2 for c in rows if c.kernel == "qkv_attention<%d,2>" % ch}
        assert par == {0, 1}, ch
        assert all(c.t <= 64 or c.n * c.heads * ((c.t + 63) // 64) > 1024 for c in rows if c.kernel == "qkv_attention<%d,1>" % ch)
    assert any(c.entry == "fwd" and c.n * c.heads * ((c.t + 63) // 64) > 1024 for c in rows)
    assert any(c.entry == "ws" and c.t < 64 for c in rows)
    assert any(c.inp == "dom_last" and c.t % 64 and c.t > 1000 for c in rows)                      # long T, ragged last block
    assert any(c.kernel.endswith("/s8") and ((c.t + 63) // 64) % 8 for c in rows)                  # blocks do not divide evenly
    assert any(c.n > 1 and c.heads > 1 for c in rows)
    for ch in K.WS_UNSERVED_WIDTHS:
        assert K.launch_qkv_attention_ws(1, 64, 8, ch) == (None, 0)


@pytest.mark.parametrize("case", K.LIN_CASES, ids=_ids(K.LIN_CASES))
def test_small_linear_rows_reach_the_kernel_in_their_id(case):
    assert K.launch_small_linear(case.n, case.k, case.m, case.woff % 4 == 0) == case.kernel
    assert case.id.startswith(case.kernel)


def test_small_layer_tables_cover_the_listed_edges():
    rows = K.LIN_CASES
    both = lambda pred: {c.kernel for c in rows if pred(c)}    # noqa: E731
    assert {c.kernel for c in rows} == set(K.LIN_KERNELS)
    assert {c.m for c in rows} >= {4095, 4096} and {c.k for c in rows} >= {3072, 3076}
    assert any(c.woff % 4 for c in rows)
    assert {c.n for c in rows} >= {1, 4, 5, 8, 9}
    assert both(lambda c: not c.bias) == set(K.LIN_KERNELS) and both(lambda c: c.silu) == set(K.LIN_KERNELS)
    assert both(lambda c: not c.silu) == set(K.LIN_KERNELS)
    assert any(c.kernel == "small_linear" and c.m % 16 for c in rows)
    assert any(c.kernel == "small_linear" and c.m > 8192 * 16 for c in rows)
    assert {d % 2 for _, _, d in K.TS_CASES} == {0, 1} and any(n > len(K.TS_VALUES) for _, n, _ in K.TS_CASES)
    for up in (0, 1):
        blocks = [K.resample_blocks(u, n, h, w, c) for _, u, n, h, w, c in K.RESAMPLE_CASES if u == up]
        assert min(blocks) < 4096 < max(blocks)
    assert any(u and h % 2 and w % 2 for _, u, n, h, w, c in K.RESAMPLE_CASES)
    assert any(not u and h == 2 and w == 2 for _, u, n, h, w, c in K.RESAMPLE_CASES)
    assert any(c == 4 for _, u, n, h, w, c in K.RESAMPLE_CASES)
    assert any(cpad > c for _, c, _, _, cpad in K.NCHW_PAD_CASES)


def _reference_meets_gate(build, case, ill):
    t0 = time.perf_counter()
    d = build(case)
    seconds = time.perf_counter() - t0
    bound, e_ref, scale = K.gate(d["ref64"], d["ref32"], ill)
    print("%s: e_ref %.3g  bound %.3g  scale %.3g  %.2f s" % (case.id, e_ref, bound, scale, seconds))
    assert bool(torch.isfinite(d["ref64"]).all())
    assert e_ref <= bound, (case.id, e_ref, bound)
    assert seconds < REF_SECONDS, (case.id, seconds)
    return e_ref, bound


@pytest.mark.parametrize("case", K.GN_CASES, ids=_ids(K.GN_CASES))
def test_group_norm_fp32_reference_meets_the_gate(case):
    _reference_meets_gate(K.gn_build, case, case.ill)


@pytest.mark.parametrize("case", K.GN_PARTIAL_CASES, ids=_ids(K.GN_PARTIAL_CASES))
def test_group_norm_partial_fp32_reference_meets_the_gate(case):
    _reference_meets_gate(K.gn_partial_build, case, False)


@pytest.mark.parametrize("case", K.ATTN_CASES, ids=_ids(K.ATTN_CASES))
def test_attention_fp32_reference_meets_the_gate(case):
    _reference_meets_gate(K.attn_build, case, case.ill)


@pytest.mark.parametrize("case", K.LIN_CASES, ids=_ids(K.LIN_CASES))
def test_small_linear_fp32_reference_meets_the_gate(case):
    _reference_meets_gate(K.lin_build, case, False)


def test_constant_group_reference_is_beta_through_film_and_silu():
    case = next(c for c in K.GN_CASES if c.inp == "const" and c.kernel == "gn_fused<2>")
    d = K.gn_build(case)
    cpg = case.c // case.groups
    t = d["beta"][:cpg].double()
    f = d["film"][0].double()
    t = t * (1 + f[:cpg]) + f[case.c:case.c + cpg]
    t = t / (1 + torch.exp(-t))
    assert float((d["ref64"][0, :, :cpg] - t).abs().max()) < 1e-12


def test_timestep_and_resampling_references():
    for name, n, dim in K.TS_CASES:
        t = K.ts_input(n)
        r64, r32 = K.ts_ref(t, dim, torch.float64), K.ts_ref(t, dim, torch.float32)
        assert r64.shape == (n, dim)
        if dim % 2:
            assert bool((r64[:, -1] == 0).all())
        bound, e_ref, _ = K.gate(r64, r32, True)
        assert e_ref <= bound
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 4, 6, 8, generator=g)
    assert torch.equal(K.resample_ref(x, 1, torch.float32), K.resample_ref(x, 1, torch.float64).float())   # copies: exact
    e, s = K.err_and_scale(K.resample_ref(x, 0, torch.float32), K.resample_ref(x, 0, torch.float64))
    assert e <= K.TOL_POOL * s
