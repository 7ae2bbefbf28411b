"""The U-Net decoder's slice-invariant terms (s3d_unet_encode_fwd): the products of an up stage's first 3x3 convolution
over the skip half of its input channels do not depend on the slice, so they are computed once per image and the per-slice
convolution over the up half starts its accumulators at them (ConvLaunch::pre).

 CPU:  the algebra in float64 — split of the first 3x3 by input-channel half, and the weights-only part of trans_c / up1
       (latent = A[b] + v[s];  up1's first pre-activation = P[b] + T[s][cls(y)][cls(x)] with a 4 x 4 table per slice).
 GPU:  the whole pyramid and slices_rec against the float64 oracle (no pixel probe) at shapes that reach every kernel the
       per-image and per-slice launches take (2 x 2 .. 64 x 64 maps, 1 / 5 / 12 slices), bit-equality of a batch item with
       its own encode, run-to-run equality, and a weight update between two encodes.
Gate of the oracle comparisons: the one tests/test_gpu_parity.py uses for pyramid levels, 1e-4 * max(1, |ref|max)."""
import pytest
import torch
import torch.nn.functional as F

PRECS = ("f32", "f16x3")
PFX = "slices_generator."


# --------------------------------------------------------------------------------------------------------------------
# CPU: the decomposition in float64
# --------------------------------------------------------------------------------------------------------------------
def _cls(i, r):
    return 0 if i == 0 else 3 if i == r - 1 else 1 if i % 2 else 2


@pytest.mark.parametrize("r5", [1, 2, 3, 5])
def test_up1_decomposition_float64(r5):
    """Gate 1e-10: float64 rounding of sums of a few hundred O(1) products is ~1e-12 at these magnitudes."""
    g = torch.Generator().manual_seed(r5)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    b, ns, cx, ce, cl, ct = 2, 3, 12, 5, 8, 4            # images, slices, x5 / embedding / latent channels, Ct
    x5, emb = rn(b, cx, r5, r5), rn(ns, ce)
    wc, bc = rn(cl, cx + ce, 1, 1) * 0.3, rn(cl)
    wt, bt = rn(cl, ct, 2, 2) * 0.3, rn(ct)
    w1 = rn(ct, 2 * ct, 3, 3) * 0.3
    proj = rn(b, ct, 2 * r5, 2 * r5)
    tile = lambda t: t[:, None].expand(-1, ns, -1, -1, -1).reshape(b * ns, *t.shape[1:])
    # reference composition (unet_custom.py:50-60, unet_parts.py:55-75)
    emb_t = emb.view(1, ns, ce, 1, 1).expand(b, ns, ce, r5, r5).reshape(b * ns, ce, r5, r5)
    latent = F.conv2d(torch.cat([tile(x5), emb_t], 1), wc, bc)
    up = F.conv_transpose2d(latent, wt, bt, stride=2)
    ref = F.conv2d(torch.cat([tile(proj), up], 1), w1, None, padding=1)
    # (1) split by input-channel half: the skip half once per image
    p_skip = F.conv2d(proj, w1[:, :ct], None, padding=1)
    half = tile(p_skip) + F.conv2d(up, w1[:, ct:], None, padding=1)
    assert (half - ref).abs().max() < 1e-10
    # (2) latent = A[b] + v[s]
    a = F.conv2d(x5, wc[:, :cx], None)
    v = emb @ wc[:, cx:, 0, 0].t() + bc
    lat2 = (a[:, None] + v.view(1, ns, cl, 1, 1)).reshape(b * ns, cl, r5, r5)
    assert (lat2 - latent).abs().max() < 1e-10
    # (3) up1's first pre-activation = P[b] + T[s][cls(y)][cls(x)]: T from a 2 x 2 constant latent -> 4 x 4
    p = p_skip + F.conv2d(F.conv_transpose2d(a, wt, None, stride=2), w1[:, ct:], None, padding=1)
    t = F.conv2d(F.conv_transpose2d(v.view(ns, cl, 1, 1).expand(ns, cl, 2, 2), wt, bt, stride=2), w1[:, ct:], None, padding=1)
    r = 2 * r5
    ci = torch.tensor([_cls(i, r) for i in range(r)])
    e = t[:, :, ci][:, :, :, ci]                                  # (ns, ct, r, r)
    got = (p[:, None] + e[None]).reshape(b * ns, ct, r, r)
    assert (got - ref).abs().max() < 1e-10


# --------------------------------------------------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------------------------------------------------
_models = {}


def _model(ns, prec):
    from slice3d_amd.models import Slices3DRegModel
    from slice3d_amd.weights import load_seeded
    if (ns, prec) not in _models:
        m = load_seeded(Slices3DRegModel(n_slices=ns, mode="test", prec=prec), 0)
        _models[(ns, prec)] = m.cuda().eval()
    return _models[(ns, prec)]


def _image(b, s, seed):
    return torch.randn(b, 3, s, s, generator=torch.Generator().manual_seed(seed)) * 0.5


def _oracle64(model, img, ns):
    from oracle import ref_cpu
    sd = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu())
          for k, v in model.state_dict().items() if k.startswith(PFX)}
    with torch.no_grad():
        return ref_cpu.unet_forward(sd, img.double(), ns)


def _encode(model, img):
    code = model.encode({"img_input": img.cuda()}, want_slices=True, build_latent=False)
    return [p.permute(0, 3, 1, 2) for p in code.pyramid], code.slices_rec_flat


def _assert_matches(got, ref, what):
    feats, rec = got
    rfeats, rrec = ref
    for l, (f, r) in enumerate(list(zip(feats, rfeats)) + [(rec, rrec)]):
        assert tuple(f.shape) == tuple(r.shape), (what, l)
        err = float((f.cpu().double() - r).abs().max())
        gate = 1e-4 * max(1.0, float(r.abs().max()))
        print("%s level %d: max|err| %.3e (gate %.3e)" % (what, l, err, gate))
        assert err < gate, (what, l, err, gate)


_oracles = {}   # (b, s, ns) -> float64 oracle, shared by the two precisions


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("b,s,ns", [(2, 16, 12),    # 1 x 1 latent, 2 x 2 up1 output: first / last row and column only
                                    (3, 32, 12),
                                    (1, 48, 5),     # odd latent size, fewer than 12 slices
                                    (2, 64, 1)])    # one slice per image: the addend's image index is the image's own
def test_pyramid_and_slices_match_float64_oracle(b, s, ns, prec):
    model = _model(ns, prec)
    img = _image(b, s, 100 + s)
    if (b, s, ns) not in _oracles:
        _oracles[(b, s, ns)] = _oracle64(_model(ns, "f32"), img, ns)
    _assert_matches(_encode(model, img), _oracles[(b, s, ns)], "B%d S%d ns%d %s" % (b, s, ns, prec))


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("s", [32, 64])
def test_batch_item_equals_its_own_encode_bit_for_bit(s, prec):
    model = _model(12, prec)
    img = _image(3, s, 7 + s)
    feats, rec = _encode(model, img)
    feats2, rec2 = _encode(model, img)
    assert all(torch.equal(f, g) for f, g in zip(feats + [rec], feats2 + [rec2])), "two encodes of one input differ"
    for i in range(3):
        f1, r1 = _encode(model, img[i:i + 1])
        for l, (f, g) in enumerate(zip(feats + [rec], f1 + [r1])):
            assert torch.equal(f[12 * i:12 * (i + 1)], g), (i, l)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_weight_update_between_encodes_reaches_every_packed_term(prec):
    """Everything derived from the weights lives in the packed image, which an in-place update invalidates."""
    from slice3d_amd.models import Slices3DRegModel
    from slice3d_amd.weights import load_seeded
    model = load_seeded(Slices3DRegModel(n_slices=12, mode="test", prec=prec), 0).cuda().eval()
    img = _image(2, 32, 55)
    _encode(model, img)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        gen = model.slices_generator
        gen.emds.weight.add_(torch.randn(gen.emds.weight.shape, generator=g).cuda())
        gen.trans_c.weight.mul_(1.25)
        gen.up1.conv.double_conv[0].weight.mul_(0.8)
    _assert_matches(_encode(model, img), _oracle64(model, img, 12), "after update %s" % prec)
