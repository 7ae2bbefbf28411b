"""Conformance of the three decoder layers and fc_out against float64, on EVERY token row and on weights chosen to sit where these
kernels can go wrong: attn_layer_q_kernel, ffn_layer_f16x3_pipe_kernel<0/1>, attn_last_fused_kernel and the four-launch last layer
(prec f16x3), attn_layer_kernel, ffn_layer_kernel, attn_last_mix_kernel (prec f32), through Slices3DRegModel.encode and
decode_stages (whose capture hands out the token tensor after layers 0 and 1).  Inputs, references, weight sets and the gate are
in tests/decoder_cases.py (checked on the CPU by tests/test_decoder_cases.py); nothing here reads a file outside the repository.

Every layer is referenced from the kernels' own previous output: layer 0 from the captured fc_p | fc_s tensor, layer 1 from x0,
the last layer and fc_out from x1.  Gate of every row: max|hip - f64| <= F * max(e32, e_split) + 2^-22 * max|f64|
(decoder_cases.gate; capped by the project's absolute bounds on the seeded weights; an sdf row of fewer than 32 numbers also
counts the reference error of a fixed CPU-side population of its case).  Each row prints
`ROW id e_kernel e_ref bound` before it asserts (profiles/decoder_layers_conformance.md).  Padding lanes of a ragged group are
not compared; every real row must be finite."""
import pytest
import torch

import decoder_cases as D

pytestmark = pytest.mark.gpu

PRECS = ("f32", "f16x3")
_models = {}


def _model(ns, prec):
    from slice3d_amd.models import Slices3DRegModel
    from slice3d_amd.weights import load_seeded
    if (ns, prec) not in _models:
        m = Slices3DRegModel(img_size=D.SIZE, n_slices=ns, mode="test", prec=prec)
        load_seeded(m, 0)
        m = m.cuda().eval()
        m._decoder_cases_set = "seeded"
        _models[(ns, prec)] = m
    return _models[(ns, prec)]


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    """The ten cached models, their packed weights and workspaces (several GiB) go back to the device when the file is done: the
    suite's full-size training test that runs later needs 110 GiB in one piece."""
    yield
    import gc
    _models.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _use(model, name):
    """Put the head of weight set `name` into the model (the U-Net stays; the next encode packs the new head)."""
    if model._decoder_cases_set != name:
        params = dict(model.named_parameters())
        with torch.no_grad():
            for k, v in D.weight_set(name).items():
                params[k].copy_(v)
        model._decoder_cases_set = name


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _decode(b, q, ns, name, prec, twice=True):
    """-> (stages of one call, stages of a second call or None, decode_sdf's result)."""
    model = _model(ns, prec)
    _use(model, name)
    code = model.encode({k: v.cuda() for k, v in D.feed(b, ns).items()})
    qry = D.queries(b, q, ns).cuda()
    st = {k: v.clone() for k, v in model.decode_stages(qry, code).items()}
    st2 = model.decode_stages(qry, code) if twice else None
    sdf = model.decode_sdf(qry, code)
    torch.cuda.synchronize()
    return st, st2, sdf


def _picker(sel):
    if sel is None:
        return lambda t: t.reshape((-1,) + tuple(t.shape[2:])).cpu()
    ob, qi = torch.from_numpy(sel[0]).cuda(), torch.from_numpy(sel[1]).cuda()
    return lambda t: t[ob, qi].cpu()


def _layer_rows(tag, st, name, ns, prec, sel=None, families=D.FAMILIES):
    """The rows of one decode: [(row id, family, kernel output, (ref64, ref32, ref_split), n_slices, prec)], every layer
    referenced from the kernels' own previous output."""
    pick = _picker(sel)
    x0, x1 = pick(st["x0"]), pick(st["x1"])
    rows = []
    if "x0" in families:
        x_in = torch.cat([pick(st["fc_p"]).unsqueeze(1), pick(st["fc_s"])], 1)
        rows.append(("x0", x0, D.layer_refs(name, x_in, 0, prec)))
    if "x1" in families:
        rows.append(("x1", x1, D.layer_refs(name, x0, 1, prec)))
    fin = D.final_refs(name, x1, prec)
    rows += [("layer2", pick(st["layer2"]), fin["layer2"]), ("sdf", pick(st["sdf"]), fin["sdf"])]
    return [("%s-%s" % (tag, fam), fam, out, refs, ns, prec) for fam, out, refs in rows]


def _judge(rows, name):
    """Print every row, then return the failures [(row id, e_kernel, bound)]: each row against its own gate (decoder_cases.gate)."""
    bad = []
    print()
    for rid, fam, out, refs, ns, prec in rows:
        bound, e_ref = D.gate(refs, fam, name, ns, prec)
        e = D.err(out, refs[0])
        print("ROW %s e_kernel %.3e e_ref %.3e bound %.3e" % (rid, e, e_ref, bound))
        if not (bool(torch.isfinite(out).all()) and e <= bound):
            bad.append((rid, e, bound))
    return bad


def _chain_and_repeat(st, st2, sdf):
    """Failures of the bit-for-bit checks: the token-0 blocks are token 0 of x0 / x1, sdf is decode_sdf's, and a second call
    gives the same bits (what a wrong barrier count breaks first)."""
    bad = []
    for l in range(2):
        if not _bits_equal(st["layer%d" % l], st["x%d" % l][:, :, 0]):
            bad.append("layer%d is not token 0 of x%d" % (l, l))
    if not _bits_equal(st["sdf"], sdf):
        bad.append("sdf differs from decode_sdf")
    for k in ("x0", "x1", "layer2", "sdf"):
        if not _bits_equal(st[k], st2[k]):
            bad.append("%s differs between two calls" % k)
    return bad


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", D.WEIGHT_SETS)
@pytest.mark.parametrize("ns", D.GRID_NS)
def test_layers_match_fp64_on_every_token_row(ns, name, prec):
    """B = 2, Q in {1, 17, 250} (ragged group tails), T = n_slices + 1 in {2, 3, 8, 9, 13}: the attention kernel's minimum,
    both sides of its `wide` switch and the full token count.  x0 and x1 on all T token rows of every real query, the capture's
    full-row `layer2` and the product kernel's `sdf` (LayerNorm fold + fc_out fused), each isolated; then the chain and the
    run-to-run equalities, for the three query counts in turn."""
    rows, bits = [], []
    for q in D.GRID_Q:
        st, st2, sdf = _decode(D.GRID_B, q, ns, name, prec)
        rows += _layer_rows("dec-%s-ns%d-q%d-%s" % (name, ns, q, prec), st, name, ns, prec)
        bits += [(q, b) for b in _chain_and_repeat(st, st2, sdf)]
    bad = _judge(rows, name)
    assert not bad, bad
    assert not bits, bits


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", D.SECOND_SETS)
@pytest.mark.parametrize("ns", D.SECOND_NS)
def test_layers_match_fp64_on_a_workgroups_second_item(ns, name, prec):
    """B = 9, Q = 4000: 2250 groups = 4500 attention items for 4096 workgroups, so 404 workgroups run a second item with the
    other barrier counts (T = 13; T = 8 keeps the narrow form on both).  The references decode the first 32 groups and every
    second group from 2048 on (decoder_cases.second_item_subset); the bit-for-bit checks cover every row."""
    sel = D.second_item_subset(D.SECOND_B, D.SECOND_Q)
    st, st2, sdf = _decode(D.SECOND_B, D.SECOND_Q, ns, name, prec)
    bits = _chain_and_repeat(st, st2, sdf)
    bad = _judge(_layer_rows("second-%s-ns%d-%s" % (name, ns, prec), st, name, ns, prec, sel=sel[:2]), name)
    assert not bad, bad
    assert not bits, bits


@pytest.mark.parametrize("name", ["sharp", "small"])
@pytest.mark.parametrize("ns", [1, 7, 12])
def test_f16x3_last_layer_forms_agree_and_match_fp64(ns, name):
    """attn_last_fused_kernel (s3d_decode_set_last_fused(1), the default) and the four-launch form (0) on the weights that
    stress the exp2 softmax and the folded LayerNorm: the same bits, and each within the gate."""
    from slice3d_amd import _lib as L
    lib = L.load()
    got, rows = [], []
    try:
        for fused in (0, 1):
            assert lib.s3d_decode_set_last_fused(fused) == 0
            st, _, sdf = _decode(D.GRID_B, 250, ns, name, "f16x3", twice=False)
            got.append(st)
            rows += _layer_rows("last-%s-ns%d-%s" % (name, ns, "fused" if fused else "4launch"), st, name, ns, "f16x3",
                                families=("layer2", "sdf"))
            assert _bits_equal(st["sdf"], sdf)
    finally:
        lib.s3d_decode_set_last_fused(1)
    bad = _judge(rows, name)
    assert not bad, bad
    for k in ("x1", "layer2", "sdf"):
        assert _bits_equal(got[0][k], got[1][k]), k
