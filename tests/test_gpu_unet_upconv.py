"""up2 .. up4 of the U-Net decoder (s3d_unet_encode_fwd): ConvTranspose2d(C -> C/2, 2x2, stride 2) and the up half of the first
3x3 that follows it run as ONE convolution of the low-resolution map (ConvLaunch::up2x) — per output parity (py, px) a 2x2
convolution with weights Wc composed at pack time, plus the ConvT bias through a border-class table Tb.

 CPU:  the composition in float64 — Wc per parity, Tb per (row class, column class) — against
       conv2d(conv_transpose2d(x, Wt, bt, stride=2), W1, padding=1).
 GPU:  the whole pyramid and slices_rec against the float64 oracle (every pixel) at shapes that reach first / last rows only,
       ragged tiles, fewer than 12 slices and several tiles per image; run-to-run and batch-item bit equality; a weight update
       of the three tensors the composed operator is built from between two encodes.
Gate of the oracle comparisons: the one tests/test_gpu_parity.py uses for pyramid levels, 1e-4 * max(1, |ref|max)."""
import pytest
import torch
import torch.nn.functional as F

PRECS = ("f32", "f16x3")
PFX = "slices_generator."


# --------------------------------------------------------------------------------------------------------------------
# CPU: the composition in float64
# --------------------------------------------------------------------------------------------------------------------
def compose(wt, bt, w1):
    """wt (C, Ct, 2, 2), bt (Ct), w1 (Co, Ct, 3, 3) -> Wc (2, 2, 2, 2, C, Co) indexed [py][px][a][b][ci][co], Tb (3, 3, Co)."""
    c, ct = wt.shape[:2]
    co = w1.shape[0]
    wc = torch.zeros(2, 2, 2, 2, c, co, dtype=wt.dtype)
    for py in range(2):
        for px in range(2):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    a, b = (py + dy) // 2 - (py - 1), (px + dx) // 2 - (px - 1)      # floor division: -1 // 2 == -1
                    wc[py, px, a, b] += torch.einsum("im,om->io", wt[:, :, (py + dy) % 2, (px + dx) % 2], w1[:, :, dy + 1, dx + 1])
    tb = torch.zeros(3, 3, co, dtype=wt.dtype)
    taps = {0: (0, 1), 1: (-1, 0, 1), 2: (-1, 0)}                                     # in-bounds taps of a first / interior / last row
    for cy in range(3):
        for cx in range(3):
            for dy in taps[cy]:
                for dx in taps[cx]:
                    tb[cy, cx] += w1[:, :, dy + 1, dx + 1] @ bt
    return wc, tb


def apply_composed(x, wc, tb):
    """x (N, C, R, R) -> (N, Co, 2R, 2R): out[2r + py, 2c + px] = Tb[cls] + sum_ab x[r + py - 1 + a, c + px - 1 + b] . Wc[py, px, a, b]."""
    n, _, r, _ = x.shape
    co = wc.shape[-1]
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.zeros(n, co, 2 * r, 2 * r, dtype=x.dtype)
    for py in range(2):
        for px in range(2):
            acc = torch.zeros(n, co, r, r, dtype=x.dtype)
            for a in range(2):
                for b in range(2):
                    win = xp[:, :, py + a:py + a + r, px + b:px + b + r]               # padded index = (r + py - 1 + a) + 1
                    acc += torch.einsum("nihw,io->nohw", win, wc[py, px, a, b])
            out[:, :, py::2, px::2] = acc
    cls = torch.tensor([0 if i == 0 else 2 if i == 2 * r - 1 else 1 for i in range(2 * r)])
    return out + tb[cls][:, cls].permute(2, 0, 1)[None]


@pytest.mark.parametrize("rp", [1, 2, 3, 5])
def test_composed_upconv_float64(rp):
    """Gate 1e-10: float64 rounding of sums of a few hundred O(1) products is ~1e-12 at these magnitudes."""
    g = torch.Generator().manual_seed(10 + rp)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    n, c, ct, co = 2, 6, 3, 5
    x = rn(n, c, rp, rp)
    wt, bt, w1 = rn(c, ct, 2, 2) * 0.5, rn(ct), rn(co, ct, 3, 3) * 0.5
    ref = F.conv2d(F.conv_transpose2d(x, wt, bt, stride=2), w1, None, padding=1)
    wc, tb = compose(wt, bt, w1)
    got = apply_composed(x, wc, tb)
    assert tuple(got.shape) == tuple(ref.shape)
    assert (got - ref).abs().max() < 1e-10
    # the two parts on their own: Wc against the bias-free pair, Tb against the pair over a zero map
    ref0 = F.conv2d(F.conv_transpose2d(x, wt, None, stride=2), w1, None, padding=1)
    assert (apply_composed(x, wc, torch.zeros_like(tb)) - ref0).abs().max() < 1e-10
    refb = F.conv2d(F.conv_transpose2d(torch.zeros_like(x), wt, bt, stride=2), w1, None, padding=1)
    assert (apply_composed(torch.zeros_like(x), wc, tb) - refb).abs().max() < 1e-10


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
@pytest.mark.parametrize("b,s,ns", [(2, 16, 12),    # up2 input 2 x 2: every output row is a first or a last row
                                    (3, 32, 12),
                                    (1, 48, 5),     # odd low-res sizes, ragged tiles, fewer than 12 slices
                                    (2, 64, 1)])    # up4 output 64 x 64: several tiles both ways; the addend's image is the image's own
def test_pyramid_and_slices_match_float64_oracle(b, s, ns, prec):
    model = _model(ns, prec)
    img = _image(b, s, 200 + s)
    if (b, s, ns) not in _oracles:
        _oracles[(b, s, ns)] = _oracle64(_model(ns, "f32"), img, ns)
    _assert_matches(_encode(model, img), _oracles[(b, s, ns)], "B%d S%d ns%d %s" % (b, s, ns, prec))


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("s", [32, 64])
def test_encodes_repeat_and_batch_items_stand_alone_bit_for_bit(s, prec):
    model = _model(12, prec)
    img = _image(3, s, 17 + s)
    feats, rec = _encode(model, img)
    feats2, rec2 = _encode(model, img)
    assert all(torch.equal(f, g) for f, g in zip(feats + [rec], feats2 + [rec2])), "two encodes of one input differ"
    for i in range(3):
        f1, r1 = _encode(model, img[i:i + 1])
        for l, (f, g) in enumerate(zip(feats + [rec], f1 + [r1])):
            assert torch.equal(f[12 * i:12 * (i + 1)], g), (i, l)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_weight_update_reaches_the_composed_operator(prec):
    """Wc and Tb live in the packed image: an in-place update of any tensor they are built from must rebuild them."""
    from slice3d_amd.models import Slices3DRegModel
    from slice3d_amd.weights import load_seeded
    model = load_seeded(Slices3DRegModel(n_slices=12, mode="test", prec=prec), 0).cuda().eval()
    img = _image(2, 32, 56)
    _encode(model, img)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        gen = model.slices_generator
        gen.up2.up.weight.mul_(1.2)
        gen.up3.up.bias.add_(torch.randn(gen.up3.up.bias.shape, generator=g).cuda() * 0.5)
        gen.up4.conv.double_conv[0].weight.mul_(0.85)
    _assert_matches(_encode(model, img), _oracle64(model, img, 12), "after update %s" % prec)
