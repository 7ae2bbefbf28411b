"""CPU checks of tests/decoder_cases.py, the inputs / references / gates of tests/test_gpu_decoder_layers.py: the float64 layer of
that module is ref_cpu.transformer_layer, split22 is the f16x3 operand, the absorbed token-0 form of the last layer is the standard
layer, every weight set has the property that makes it a stress (on tokens the CPU oracle builds for the GPU file's own images
and queries), the second-item subset holds groups of both kinds, and the fp32 oracle alone meets every gate with margin."""
import numpy as np
import pytest
import torch

import decoder_cases as D
from oracle import ref_cpu

F64, F32 = torch.float64, torch.float32
Q_PROP = 250


def _tokens(name, ns):
    return D.cpu_tokens(name, D.GRID_B, Q_PROP, ns)


def test_float64_layer_is_the_oracles_layer():
    x = _tokens("seeded", 7).double()
    for name in ("seeded", "sharp"):
        for l in range(D.N_LAYERS):
            p = "att_decoder.layers.%d" % l
            a, b = D.layer(D.head64(name), x, p), ref_cpu.transformer_layer(D.head64(name), x, p)
            assert torch.equal(a, b), (name, l, float((a - b).abs().max()))
            x = a


def test_split22_is_the_f16x3_operand():
    g = torch.Generator().manual_seed(5)
    mag = torch.exp2(torch.rand(200000, generator=g, dtype=F64) * 20 - 4)           # 2^-4 .. 2^16
    x = (mag * torch.where(torch.rand(200000, generator=g) < 0.5, -1.0, 1.0)).float().double()
    x = x[x.abs() < D.F16_MAX]
    rel = ((D.split22(x) - x).abs() / x.abs()).max()
    print("split22: worst relative error %.3e (2^-21 = %.3e)" % (float(rel), 2.0 ** -21))
    assert float(rel) <= 2.0 ** -21
    tiny = torch.linspace(-2.0 ** -4, 2.0 ** -4, 10001, dtype=F64)
    assert float((D.split22(tiny) - tiny).abs().max()) <= 2.0 ** -25              # lo is an f16 subnormal: absolute
    big = torch.tensor([65520.0, 7e4, -1e9, float("inf")], dtype=F64)
    assert torch.equal(D.split22(big), torch.tensor([float("inf"), float("inf"), float("-inf"), float("inf")], dtype=F64))
    assert float(D.split22(torch.tensor([65504.0], dtype=F64))) == 65504.0
    h = torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -20], dtype=F64)                      # hi = 1, lo = 2^-11 + 2^-20 exactly
    assert float(D.split22(h)) == float(h)


@pytest.mark.parametrize("ns", [1, 12])
@pytest.mark.parametrize("name", D.WEIGHT_SETS)
def test_absorbed_last_layer_is_the_standard_layers_token_0(name, ns):
    x = _tokens(name, ns).double()
    p = "att_decoder.layers.%d" % (D.N_LAYERS - 1)
    probe = {}
    D.layer(D.head64(name), x, p, None, probe)
    u = D.absorbed_last_tok0(D.head64(name), x, p)
    e = float((u - probe["ln1_in"][:, 0]).abs().max())
    print("absorbed last layer %s ns%d: %.1e" % (name, ns, e))
    assert e <= 1e-11 * float(u.abs().max())


@pytest.mark.parametrize("ns", D.GRID_NS)
@pytest.mark.parametrize("name", D.WEIGHT_SETS)
def test_weight_set_properties(name, ns):
    """Every set, float64 and fp32: no inf / NaN, every split operand inside the f16x3 domain.  sharp: the median largest
    probability is > 0.9 (over the three layers) and an exponential underflows (some row's logit range exceeds 126 ln 2).
    shift (+ 64 on every out_proj.bias and linear2.bias): the mean of EVERY LayerNorm input row, all six LayerNorms, is > 20
    standard deviations — the large-mean LayerNorm stress.  offset (+ 40, fc_p.bias included, as first specified) cannot have that
    property and is kept as a second stress beside it: its row means are > 16 standard deviations (row minima 17.8 - 22.9) on five
    of the six LayerNorms, and in layer 0's first one the value rows carry
    fc_p's offset through Wv (standard deviation about 55, measured ratio 0.5), which makes that layer a softmax stress instead
    (logit range about 5 500, asserted > 1 000).  small: the median LayerNorm1 input variance of layer 0 is in
    [1e-6, 1e-4], where eps = 1e-5 decides the result."""
    x = _tokens(name, ns)
    for dt in (F64, F32):
        probes, out = D.properties(name, x, dt)
        assert bool(torch.isfinite(out).all())
        for p in probes:
            assert p["finite"] and p["operand_max"] < D.F16_MAX, (dt, p["operand_max"])
    probes, _ = D.properties(name, x, F64)
    if name == "sharp":
        pmax = torch.cat([p["att"].amax(-1).reshape(-1) for p in probes])
        rng = max(float(p["logit_range"].max()) for p in probes)
        print("sharp ns%d: median max probability %.4f, largest logit range %.1f" % (ns, float(pmax.median()), rng))
        assert float(pmax.median()) > 0.9
        if ns > 1:      # (T = 2: one competitor per row; the range is asserted where there are more)
            assert rng > 126 * np.log(2.0)
        lowest = min(float((p["att"] / p["att"].amax(-1, keepdim=True)).min()) for p in probes)
        assert ns == 1 or lowest < 2.0 ** -126
    elif name == "offset":
        lns = [u for p in probes for u in (p["ln1_in"], p["ln2_in"])]
        ratios = [float(D.row_mean_over_std(u)) for u in lns]
        medians = [float((u.mean(-1).abs() / u.std(-1, unbiased=False)).median()) for u in lns]
        print("offset ns%d: |mean| / std per LayerNorm, min %s median %s, layer-0 logit range %.0f"
              % (ns, ["%.1f" % r for r in ratios], ["%.1f" % r for r in medians], float(probes[0]["logit_range"].max())))
        assert all(r > 16.0 for r in ratios[1:]), (ratios, medians)
        assert float(probes[0]["logit_range"].max()) > 1000.0
    elif name == "shift":
        ratios = [float(D.row_mean_over_std(u)) for p in probes for u in (p["ln1_in"], p["ln2_in"])]
        print("shift ns%d: min |mean| / std per LayerNorm %s" % (ns, ["%.1f" % r for r in ratios]))
        assert len(ratios) == 6 and all(r > 20.0 for r in ratios), ratios
    elif name == "small":
        var = float(probes[0]["ln1_in"].var(-1, unbiased=False).median())
        print("small ns%d: median LayerNorm1 input variance of layer 0 %.3e" % (ns, var))
        assert 1e-6 <= var <= 1e-4


def test_second_item_subset_holds_first_and_second_item_groups():
    b, q = D.SECOND_B, D.SECOND_Q
    ob, qi, groups = D.second_item_subset(b, q)
    gpb = (q + 15) // 16
    n_groups = b * gpb
    assert n_groups == 2250 and 2 * n_groups - D.ATTN_BLOCKS == 404        # 404 workgroups run a second item
    rounds = [D.item_round(int(g), n_groups) for g in groups]
    first = [g for g, r in zip(groups, rounds) if r == (0, 0)]
    second = [g for g, r in zip(groups, rounds) if r == (1, 1)]
    assert len(first) == D.SUBSET_HEAD_GROUPS and len(second) >= 64 and len(first) + len(second) == len(groups)
    assert min(second) == D.ATTN_BLOCKS // 2 and max(second) >= n_groups - D.SUBSET_TAIL_STRIDE
    assert len(set(zip(ob.tolist(), qi.tolist()))) == len(ob) == 16 * len(groups)      # Q = 4000: no ragged group
    assert int(ob.max()) == b - 1 and int(qi.max()) < q
    assert np.array_equal(np.unique(ob * gpb + qi // 16), np.sort(groups))
    for g in (0, 2047):
        assert D.item_round(g, n_groups) == (0, 0)
    assert D.item_round(5, 8) == (0, 0)                                       # small jobs: one item per workgroup


def _gate_rows(name, x, prec):
    """The gates of the GPU file with the fp32 oracle in the kernels' place (chained from its own output)."""
    rows = []
    for l in range(D.N_LAYERS - 1):
        refs = D.layer_refs(name, x, l, prec)
        rows.append(("x%d" % l, refs))
        x = refs[1]
    fin = D.final_refs(name, x, prec)
    return rows + [("layer2", fin["layer2"]), ("sdf", fin["sdf"])]


@pytest.mark.parametrize("ns", D.GRID_NS)
@pytest.mark.parametrize("name", D.WEIGHT_SETS)
def test_fp32_oracle_meets_every_gate_with_margin(name, ns):
    """Every grid case (Q = 1, 17, 250; both precisions) through the gate the GPU file uses, the few-sample sdf rule included:
    e32 <= bound / 4.  The population figure of the sdf family is of the size of the Q = 250 row's own reference error (it is
    formed on the same 500 queries, behind fp32 instead of kernel layers), so the Q = 1 rows are held to what the Q = 250 rows are."""
    for prec in ("f32", "f16x3"):
        pop = D.sdf_population_error(name, ns, prec)
        for q in D.GRID_Q:
            for fam, refs in _gate_rows(name, D.cpu_tokens(name, D.GRID_B, q, ns), prec):
                assert D.FACTOR[fam] == D.REF_FACTOR
                bound, e_ref = D.gate(refs, fam, name, ns, prec)
                e32 = D.err(refs[1], refs[0])
                print("ROW cpu-%s-ns%d-q%d-%s-%s e32 %.3e e_ref %.3e bound %.3e" % (name, ns, q, prec, fam, e32, e_ref, bound))
                assert e32 <= bound / 4, (fam, prec, q, e32, bound)
                own = D.ref_error(refs)
                if fam == "sdf" and q == 1:
                    assert refs[0].numel() < D.SDF_MIN_SAMPLES and e_ref == max(own, pop)
                else:
                    assert e_ref == own                                   # every other row: the issue's formula as it stands
                if fam == "sdf" and q == D.POP_Q:
                    assert 0.25 * own <= pop <= 4.0 * own, (pop, own)     # the population is this case


@pytest.mark.parametrize("name", D.SECOND_SETS)
def test_fp32_oracle_meets_the_second_item_gates(name):
    ob, qi, _ = D.second_item_subset(D.SECOND_B, D.SECOND_Q)
    keep = np.arange(0, len(ob), 8)                                          # (an eighth of the subset: the CPU stays quick)
    x = D.cpu_tokens(name, D.SECOND_B, D.SECOND_Q, D.SECOND_NS[-1], sel=(ob[keep], qi[keep]))
    assert x.shape == (len(keep), D.SECOND_NS[-1] + 1, 128)
    for fam, refs in _gate_rows(name, x, "f16x3"):
        bound, _ = D.gate(refs, fam, name, D.SECOND_NS[-1], "f16x3")
        assert D.err(refs[1], refs[0]) <= bound / 4, fam
