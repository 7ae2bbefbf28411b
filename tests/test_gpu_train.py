"""GPU tests of the training step (s3d_train_fwd_bwd / s3d_adam_step through the C ABI) against
(1) golden losses/gradients/running statistics captured from the REAL reference in train mode
    (dropout pinned to 0), and (2) autograd through the CPU oracle on other shapes.
Gradient tolerance: the L1 losses make d loss/d x = sign(.)/n, so two fp32 evaluations disagree on a few
signs of near-zero residuals; gradients are compared by relative L2 error per tensor (<= 2e-2, typical
1e-3) and losses to 1e-5 relative."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, load_golden, seeded_sd_from_shapes

pytestmark = pytest.mark.gpu

# conv biases directly in front of a train-mode BatchNorm: their exact gradient is 0 (BN removes the
# mean), what both implementations produce is rounding noise
PRE_BN_BIASES = {"slices_generator.%s.bias" % k for k in
                 ("down1.0", "down2.7", "down3.14", "down3.17", "down4.24", "down4.27", "down5.34", "down5.37")}


def _shapes(n_slices):
    shapes = {k: tuple(v) for k, v in json.load(open(os.path.join(GOLDEN, "state_dict_keys.json"))).items()}
    shapes["slices_generator.emds.weight"] = (n_slices, 128)
    return shapes


def make_trainer(ns, prec="f32"):
    from slice3d_amd.models import Slices3DRegModel
    from slice3d_amd.trainer import HipTrainer
    from slice3d_amd.weights import load_seeded
    m = load_seeded(Slices3DRegModel(n_slices=ns, mode="train"), 0).cuda()
    return m, HipTrainer(m, prec=prec)


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_train_step_matches_reference_golden(prec):
    z = np.load(os.path.join(GOLDEN, "g5_train_s32_n12_q128_b2.npz"))
    m, tr = make_trainer(12, prec)
    batch = {k: torch.from_numpy(z[k]).cuda() for k in
             ("img_input", "img_slices", "qry_norot", "sdf", "obj_rot_mat", "trans_mat_wo_rot_tp")}
    losses, sdf_pred, rec = tr.forward_backward(batch, want_outputs=True)
    torch.cuda.synchronize()
    got = losses.cpu().numpy().astype(np.float64)
    want = z["losses"]
    assert np.abs(sdf_pred.cpu().numpy() - z["sdf_pred"]).max() < 1e-4
    for i in range(3):
        assert abs(got[i] - want[i]) < 2e-5 * abs(want[i]) + 1e-7, (i, got[i], want[i])
    assert abs(got[3] - want[3]) < 1e-6
    sd = dict(m.named_parameters())
    worst = 0.0
    for k in z["grad_names"]:
        k = str(k)
        g = sd[k].grad.reshape(-1).cpu().numpy()
        norm, gmax = z["gn:" + k]
        if k in PRE_BN_BIASES:
            assert np.abs(g).max() < 1e-4
            continue
        assert abs(np.linalg.norm(g) - norm) < 2e-2 * norm, (k, np.linalg.norm(g), norm)
        idx, val = z["gi:" + k], z["gv:" + k]
        err = np.abs(g[idx] - val).max() / gmax
        worst = max(worst, err)
        assert err < 2e-2, (k, err)
    for key in z.files:
        if key.startswith("bn:") and ".down5_." not in key:
            got_stat = m.state_dict()[key[3:]].cpu().numpy()
            assert np.abs(got_stat - z[key]).max() < 1e-5, key
    print("worst sampled-gradient error / max|g| = %.2e" % worst)


# q >= 4096 exercises the locality-sorted token order (s3d_query_sort) and the tiled sampling backward
@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("b,s,q,ns", [(1, 32, 50, 12), (2, 48, 33, 4), (2, 32, 4200, 3)])
def test_train_grads_match_oracle_autograd(b, s, q, ns, prec):
    from oracle import ref_cpu
    from slice3d_amd.synth import make_feed_dict
    m, tr = make_trainer(ns, prec)
    fd = make_feed_dict(b, s, q, ns, seed=200 + q)
    sd = seeded_sd_from_shapes(_shapes(ns))
    for k, v in sd.items():
        if v.is_floating_point() and "running" not in k and not k.startswith("vggptlossfunc"):
            v.requires_grad_(True)
    loss, parts, out, ts = ref_cpu.forward_train(sd, fd, ns, 0.0)
    loss.backward()
    losses = tr.forward_backward({k: v.cuda() for k, v in fd.items()})
    got = losses.cpu().numpy()
    for i in range(3):
        assert abs(got[i] - float(parts[i])) < 2e-5 * abs(float(parts[i])) + 1e-7
    for k, p in m.named_parameters():
        if k not in tr.offsets:
            continue
        ref = sd[k].grad
        if k in PRE_BN_BIASES:
            assert float(p.grad.abs().max()) < 1e-4
            continue
        if ref is None:
            continue
        g = p.grad.cpu()
        rel = float((g - ref).norm() / ref.norm())
        assert rel < 2e-2, (k, rel)


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_last_layer_absorbed_attention_gradients_by_projection(prec):
    """The last decoder layer trains in the absorbed token-0 form (train2.hip: M = Wk^T Wq, N = Wo Wv; models.py:83 consumes
    token 0 only) and its in_proj / out_proj gradients come out of a chain rule through those products.  Checked per
    projection block against CPU autograd of the oracle's ordinary attention: the q, k and v row blocks of in_proj_weight, the
    q and v blocks of in_proj_bias, out_proj.  The key bias cancels in the softmax: its gradient is written as exactly zero
    here and is rounding noise in the oracle."""
    from oracle import ref_cpu
    from slice3d_amd.synth import make_feed_dict
    b, s, q, ns = 2, 32, 600, 5
    m, tr = make_trainer(ns, prec)
    fd = make_feed_dict(b, s, q, ns, seed=4242)
    sd = seeded_sd_from_shapes(_shapes(ns))
    for k, v in sd.items():
        if v.is_floating_point() and "running" not in k and not k.startswith("vggptlossfunc"):
            v.requires_grad_(True)
    loss, parts, out, ts = ref_cpu.forward_train(sd, fd, ns, 0.0)
    loss.backward()
    tr.forward_backward({k: v.cuda() for k, v in fd.items()})
    grads = {k: p.grad.cpu() for k, p in m.named_parameters() if k in tr.offsets}
    pre = "att_decoder.layers.2.self_attn."
    gw, rw = grads[pre + "in_proj_weight"], sd[pre + "in_proj_weight"].grad
    gb, rb = grads[pre + "in_proj_bias"], sd[pre + "in_proj_bias"].grad
    for name, sl in (("q", slice(0, 128)), ("k", slice(128, 256)), ("v", slice(256, 384))):
        rel = float((gw[sl] - rw[sl]).norm() / rw[sl].norm())
        assert rel < 2e-2, ("in_proj_weight", name, rel)
    for name, sl in (("q", slice(0, 128)), ("v", slice(256, 384))):
        rel = float((gb[sl] - rb[sl]).norm() / rb[sl].norm())
        assert rel < 2e-2, ("in_proj_bias", name, rel)
    assert float(gb[128:256].abs().max()) == 0.0
    assert float(rb[128:256].norm()) < 1e-4 * float(rb.norm())
    go, ro = grads[pre + "out_proj.weight"], sd[pre + "out_proj.weight"].grad
    for h in range(4):                                     # per head column block
        rel = float((go[:, 32 * h:32 * h + 32] - ro[:, 32 * h:32 * h + 32]).norm() / ro[:, 32 * h:32 * h + 32].norm())
        assert rel < 2e-2, ("out_proj.weight", h, rel)
    gob, rob = grads[pre + "out_proj.bias"], sd[pre + "out_proj.bias"].grad
    assert float((gob - rob).norm() / rob.norm()) < 2e-2


def test_dropout_masks_are_bernoulli_with_the_stated_rate_and_uncorrelated():
    """The counter-based masks of dropout.h (exported by s3d_dropout_mask; the kernels draw exactly these): values are 0 or
    1/(1-p), the keep rate of every 16-bit field position is 1 - p to sampling accuracy, neighbours (the four fields of one hash,
    consecutive hashes, a row stride apart) and different sites / seeds are uncorrelated, and a stream does not depend on the
    offset it is drawn from."""
    from slice3d_amd import _lib
    lib = _lib.load()
    p, n = 0.1, 1 << 22

    def draw(seed, site, idx0=0, count=n):
        out = torch.empty(count, dtype=torch.float32, device="cuda")
        _lib.check(lib.s3d_dropout_mask(seed, site, idx0, count, p, out.data_ptr(), None), "s3d_dropout_mask")
        torch.cuda.synchronize()
        return out

    m = draw(12345678901, 6)
    vals = torch.unique(m).cpu().tolist()
    assert len(vals) == 2 and vals[0] == 0.0 and abs(vals[1] - 1.0 / (1.0 - p)) < 1e-6, vals
    k = (m > 0).double()
    sigma = (p * (1 - p) / n) ** 0.5
    assert abs(float(k.mean()) - (1 - p)) < 5 * sigma, float(k.mean())
    for f in range(4):                                    # the four fields of a hash word pair
        assert abs(float(k[f::4].mean()) - (1 - p)) < 5 * 2 * sigma, (f, float(k[f::4].mean()))
    kc = k - k.mean()
    var = float((kc * kc).mean())
    for lag in (1, 2, 3, 4, 128, 2048):                   # inside a hash, the next hash, a channel row, a hidden row
        c = float((kc[:-lag] * kc[lag:]).mean()) / var
        assert abs(c) < 5 / n ** 0.5, (lag, c)
    for other in (draw(12345678901, 7), draw(12345678902, 6)):   # another site, another seed
        oc = (other > 0).double()
        c = float(((oc - oc.mean()) * kc).mean()) / var
        assert abs(c) < 5 / n ** 0.5, c
    off = 1000003                                          # the same stream drawn from an offset (and past 2^32 elements)
    assert torch.equal(draw(12345678901, 6, off, 4096), m[off:off + 4096])
    hi = draw(12345678901, 6, (1 << 33) + 5, 1 << 16)
    assert abs(float((hi > 0).double().mean()) - (1 - p)) < 5 * (p * (1 - p) / (1 << 16)) ** 0.5


def _hip_dropout_masks(b, q, ns, p, seed):
    """Rebuild, in the oracle's (query, token, ...) layout, the masks the HIP kernels draw (s3d_dropout_mask)."""
    import ctypes as C
    from slice3d_amd import _lib
    lib = _lib.load()
    T = ns + 1
    gpb = (q + 15) // 16
    G = gpb * b
    rows, rows0 = G * T * 16, G * 16
    qi = torch.arange(q)
    masks = []
    for l in range(3):
        def gen(site, n):
            out = torch.empty(n, dtype=torch.float32, device="cuda")
            _lib.check(lib.s3d_dropout_mask(seed, 4 * l + site, 0, n, p, out.data_ptr(), None), "s3d_dropout_mask")
            torch.cuda.synchronize()
            return out.cpu()
        # row of (batch bb, query q, token t) in the token tensor
        row = torch.stack([torch.stack([((bb * gpb + qi // 16) * T + t) * 16 + qi % 16 for t in range(T)], 1)
                           for bb in range(b)]).reshape(b * q, T)                       # (R, T)
        if l < 2:
            m_att = gen(0, rows * 4 * 16).view(rows, 4, 16)[row][:, :, :, :T].permute(0, 2, 1, 3)   # (R, 4, Tq, Tk)
            m_o = gen(1, rows * 128).view(rows, 128)[row]                                             # (R, T, 128)
            m_h = gen(2, rows * 2048).view(rows, 2048)[row]
            m_f = gen(3, rows * 128).view(rows, 128)[row]
        else:   # only token 0 of the last layer is consumed: all four of its sites index the compact token-0 rows
            row0 = torch.cat([(bb * gpb + qi // 16) * 16 + qi % 16 for bb in range(b)])
            m_att = torch.ones(b * q, 4, T, T)
            m_o = torch.ones(b * q, T, 128)
            m_h = torch.ones(b * q, T, 2048)
            m_f = torch.ones(b * q, T, 128)
            m_att[:, :, 0, :] = gen(0, rows0 * 4 * 16).view(rows0, 4, 16)[row0][:, :, :T]
            m_o[:, 0] = gen(1, rows0 * 128).view(rows0, 128)[row0]
            m_h[:, 0] = gen(2, rows0 * 2048).view(rows0, 2048)[row0]
            m_f[:, 0] = gen(3, rows0 * 128).view(rows0, 128)[row0]
        masks.append({"att": m_att, "o": m_o, "h": m_h, "f": m_f})
    return masks


def test_dropout_matches_oracle_with_identical_masks():
    """Train step with dropout 0.1: the oracle is run with the very masks the kernels generate
    (counter-based, exported through s3d_dropout_mask), so losses and gradients must agree as at p = 0."""
    from oracle import ref_cpu
    from slice3d_amd.synth import make_feed_dict
    b, s, q, ns, p = 1, 32, 40, 12, 0.1
    m, tr = make_trainer(ns)
    tr.dropout = p
    fd = make_feed_dict(b, s, q, ns, seed=321)
    losses = tr.forward_backward({k: v.cuda() for k, v in fd.items()})
    got = losses.cpu().numpy()
    masks = _hip_dropout_masks(b, q, ns, p, tr.last_seed)
    keep = float(masks[0]["h"].gt(0).float().mean())
    assert abs(keep - (1 - p)) < 0.01, keep
    assert float(masks[0]["h"].max()) == pytest.approx(1 / (1 - p))
    sd = seeded_sd_from_shapes(_shapes(ns))
    for k, v in sd.items():
        if v.is_floating_point() and "running" not in k and not k.startswith("vggptlossfunc"):
            v.requires_grad_(True)
    loss, parts, out, ts = ref_cpu.forward_train(sd, fd, ns, p, masks=masks)
    loss.backward()
    for i in range(3):
        assert abs(got[i] - float(parts[i])) < 2e-5 * abs(float(parts[i])) + 1e-7, (i, got[i], float(parts[i]))
    for k, prm in m.named_parameters():
        if k not in tr.offsets or k in PRE_BN_BIASES or sd[k].grad is None:
            continue
        rel = float((prm.grad.cpu() - sd[k].grad).norm() / sd[k].grad.norm())
        assert rel < 2e-2, (k, rel)
    # and the dropout run differs from the p = 0 run (the masks are really applied)
    tr.dropout = 0.0
    l0 = tr.forward_backward({k: v.cuda() for k, v in fd.items()}).cpu().numpy()
    assert abs(l0[0] - got[0]) > 1e-4


# (20000 queries, 64^2): loss gradients of 5e-5 (sdf) and 7e-6 (images) per element — far below f16's normal range;
# the backward scale (api_train.inc backward_scale) must keep the split-precision GEMMs exact there too
@pytest.mark.parametrize("p_drop,q", [(0.0, 200), (0.1, 200), (0.0, 20000)])
def test_f16x3_training_gemms_match_fp32(p_drop, q):
    """prec='f16x3' routes the forward / data-gradient GEMMs of the train step through the split-precision
    kernels (fused FFN forward / backward, conv engine; weight gradients stay fp32): losses and gradients must
    agree with the fp32 run to fp32 noise — with dropout too, since both paths draw the same counter-based masks."""
    from slice3d_amd.models import Slices3DRegModel
    from slice3d_amd.synth import make_feed_dict
    from slice3d_amd.trainer import HipTrainer
    from slice3d_amd.weights import load_seeded
    fd = {k: v.cuda() for k, v in make_feed_dict(1, 64, q, 12, seed=77).items()}
    res = {}
    for prec in ("f32", "f16x3"):
        m = load_seeded(Slices3DRegModel(n_slices=12, mode="train"), 0).cuda()
        tr = HipTrainer(m, prec=prec, dropout=p_drop, seed=5)
        losses = tr.forward_backward(fd).cpu().numpy().copy()
        res[prec] = (losses, tr.grad_flat.cpu().clone(), tr)
    la, lb = res["f32"][0], res["f16x3"][0]
    for i in range(3):
        assert abs(la[i] - lb[i]) < 2e-5 * abs(la[i]) + 1e-7, (i, la[i], lb[i])
    ga, gb, tr = res["f32"][1], res["f16x3"][1], res["f32"][2]
    assert float((ga - gb).norm() / ga.norm()) < 2e-2
    gmax = max(float(ga[tr.offsets[k]:tr.offsets[k] + p.numel()].norm()) for k, p in zip(tr.names, tr.params))
    for k, p in zip(tr.names, tr.params):
        if k in PRE_BN_BIASES:
            continue
        off, n = tr.offsets[k], p.numel()
        a, b = ga[off:off + n], gb[off:off + n]
        # shallow encoder gradients feel the sign flips of near-zero L1 residuals most (see module docstring);
        # the absolute term covers bias gradients that are themselves a near-cancelling sum (|g| ~ 1e-4 gmax)
        assert float((a - b).norm()) < 5e-2 * float(a.norm()) + 1e-4 * gmax, k


def test_adam_step_matches_torch_adam():
    m, tr = make_trainer(12)
    torch.manual_seed(0)
    ps = [p for p in tr.params[:6]]
    ref = [p.detach().clone().cpu() for p in ps]
    opt = torch.optim.Adam([r.requires_grad_(True) for r in ref], lr=3e-4)
    for step in range(3):
        tr.grad_flat.normal_(0, 0.1)
        for r, p in zip(ref, ps):
            r.grad = p.grad.detach().cpu().clone()
        opt.step()
        tr.adam_step()
    for r, p in zip(ref, ps):
        assert (r.detach() - p.detach().cpu()).abs().max() < 1e-6


def test_training_reduces_the_loss():
    from slice3d_amd.synth import make_feed_dict
    m, tr = make_trainer(12)
    batch = {k: v.cuda() for k, v in make_feed_dict(2, 32, 256, 12, seed=8).items()}
    first = tr.train_step(batch)
    for _ in range(15):
        last = tr.train_step(batch)
    assert sum(last[:3]) < 0.8 * sum(first[:3]), (first, last)
    m.eval()
    out = m(batch)            # eval-mode forward works after training (repacks with the new running stats)
    assert torch.isfinite(out["sdf_pred"]).all()


_big_oracle = {}
BIG = dict(ns=12, s=128, q=16384, seed=777)


def _big_case_oracle():
    """Compact oracle outputs of the 128^2 x 16 384-query train step (committed: tests/golden/oracle_train_128_16k.npz,
    written by tests/golden/make_oracle_golden.py from this function; S3D_LIVE_ORACLE=1 recomputes)."""
    from helpers import compact_grads, load_oracle_golden
    if "z" not in _big_oracle:
        z = load_oracle_golden("train_128_16k")
        if z is None:
            from oracle import ref_cpu
            from slice3d_amd.synth import make_feed_dict
            fd = make_feed_dict(1, BIG["s"], BIG["q"], BIG["ns"], seed=BIG["seed"])
            sd = seeded_sd_from_shapes(_shapes(BIG["ns"]))
            for k, v in sd.items():
                if v.is_floating_point() and "running" not in k and not k.startswith("vggptlossfunc"):
                    v.requires_grad_(True)
            loss, parts, out, ts = ref_cpu.forward_train(sd, fd, BIG["ns"], 0.0)
            loss.backward()
            z = compact_grads({k: v.grad for k, v in sd.items() if v.grad is not None})
            z["parts"] = np.array([float(p) for p in parts])
            z["sdf_pred"] = out["sdf_pred"].detach().numpy()
            del loss, out, ts
        _big_oracle["z"] = z
    return _big_oracle["z"]


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_train_step_matches_oracle_autograd_128_16k(prec):
    """A train step at a size where the loss gradients are small (1/n = 6e-5 on sdf, 1.7e-6 on the slice images:
    f16-subnormal territory, the regime where the split-precision backward needs its power-of-two scale) against
    CPU autograd through the oracle: 128^2 x 12 slices x 16 384 queries, dropout 0.  Both arithmetic modes are
    compared with the same oracle gradients — not with each other.  (Oracle outputs: committed golden, per tensor the
    2 048 sampled entries of helpers.compact_grads.)"""
    from helpers import sampled_grad
    from slice3d_amd.models import Slices3DRegModel
    from slice3d_amd.synth import make_feed_dict
    from slice3d_amd.trainer import HipTrainer
    from slice3d_amd.weights import load_seeded
    ns, s, q = BIG["ns"], BIG["s"], BIG["q"]
    fd = make_feed_dict(1, s, q, ns, seed=BIG["seed"])
    z = _big_case_oracle()
    parts, sdf_ref = z["parts"], torch.from_numpy(z["sdf_pred"])
    m = load_seeded(Slices3DRegModel(n_slices=ns, mode="train"), 0).cuda()
    tr = HipTrainer(m, prec=prec)
    losses, sdf_pred, rec = tr.forward_backward({k: v.cuda() for k, v in fd.items()}, want_outputs=True)
    got = losses.cpu().numpy()
    assert (sdf_pred.cpu() - sdf_ref).abs().max() < 1e-4
    for i in range(3):
        assert abs(got[i] - parts[i]) < 2e-5 * abs(parts[i]) + 1e-7, (i, got[i], parts[i])
    worst, worst_k, names = 0.0, None, {str(k) for k in z["grad_names"]}
    for k, p in m.named_parameters():
        if k not in tr.offsets or k not in names:
            continue
        if k in PRE_BN_BIASES:
            assert float(p.grad.abs().max()) < 1e-4
            continue
        got_k = sampled_grad(z, k, p.grad)   # against the closer of the fp32 oracle passes the golden holds (GPU box's host, authoring container)
        rel = min(float(np.linalg.norm(got_k - z[t + k].astype(np.float64)) / np.linalg.norm(z[t + k].astype(np.float64)))
                  for t in ("g32:", "g32c:") if t + k in z)
        if rel > worst:
            worst, worst_k = rel, k
        assert rel < 2e-2, (k, rel)
    print("train 128^2/16k (%s): worst relative gradient error %.2e (%s)" % (prec, worst, worst_k))


def test_optimizer_state_round_trips_through_torch_adam():
    """The 'opt' checkpoint entry is torch.optim.Adam(model.parameters())'s state_dict (train.py:136,174-176): all 179
    parameters numbered in model.parameters() order, state only for tensors that got a gradient.  (1) the trainer's
    state loads into a real torch Adam over the same parameter list; (2) a torch Adam stepped with the same gradients
    produces a state the trainer loads, and both then take the same next step."""
    from slice3d_amd.synth import make_feed_dict
    m, tr = make_trainer(12)
    n_all = len(list(m.parameters()))
    assert n_all == 179 and len(tr.params) == 137
    batch = {k: v.cuda() for k, v in make_feed_dict(1, 32, 64, 12, seed=8).items()}
    # reference-side twin: CPU copies of all parameters, torch Adam over ALL of them (frozen ones never get a grad)
    twin = [p.detach().cpu().clone().requires_grad_(p.requires_grad) for p in m.parameters()]
    pos = {id(p): i for i, p in enumerate(m.parameters())}
    opt = torch.optim.Adam(twin, lr=3e-4)
    for _ in range(2):
        tr.forward_backward(batch)
        for p in tr.params:
            twin[pos[id(p)]].grad = p.grad.detach().cpu().clone()
        opt.step()
        tr.adam_step()
    sd = tr.state_dict()
    assert sorted(sd["state"]) == sorted(opt.state_dict()["state"])          # same sparse numbering
    assert sd["param_groups"][0]["params"] == list(range(n_all))
    fresh = torch.optim.Adam([t.detach().clone().requires_grad_(t.requires_grad) for t in twin], lr=1.0)
    fresh.load_state_dict(sd)                                                   # (1) torch accepts it
    for i, st in opt.state_dict()["state"].items():
        assert (sd["state"][i]["exp_avg"].cpu() - st["exp_avg"]).abs().max() < 1e-6
        assert float(sd["state"][i]["step"]) == float(st["step"]) == 2.0
    m2, tr2 = make_trainer(12)                                                  # (2) torch's state into a new trainer
    with torch.no_grad():
        for a, b in zip(m2.parameters(), m.parameters()):
            a.copy_(b)
    tr2.load_state_dict(opt.state_dict())
    assert tr2.step == 2
    tr.forward_backward(batch)
    tr2.grad_flat.copy_(tr.grad_flat)
    tr.adam_step()
    tr2.adam_step()
    for a, b in zip(tr.params, tr2.params):     # moments went through torch's CPU arithmetic: equal to fp32 rounding
        assert (a - b).abs().max() < 1e-6
    bad = opt.state_dict()
    bad["state"][0]["exp_avg"] = torch.zeros(3)
    bad["state"][0]["exp_avg_sq"] = torch.zeros(3)
    with pytest.raises(Exception):
        tr2.load_state_dict(bad)


def _reference_style_losses(out, batch):
    """train.py:29-47 written with torch ops, as a user of the reference would."""
    import torch.nn.functional as F
    return (F.l1_loss(out["sdf_pred"], batch["sdf"]), F.l1_loss(out["slices_rec"], batch["img_slices"]), out["vgg_loss"])


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_autograd_train_forward_reproduces_reference_golden(prec):
    """The reference's training contract (train.py:41-53): `model.train(); x = model(batch); loss(x).backward()` with
    the loss written in torch by the caller — through s3d_train_fwd / s3d_train_bwd behind a torch.autograd.Function.
    Outputs, losses and the gradients autograd leaves in param.grad must match the g5 goldens of the REAL reference."""
    from slice3d_amd.models import Slices3DRegModel
    from slice3d_amd.weights import load_seeded
    z = np.load(os.path.join(GOLDEN, "g5_train_s32_n12_q128_b2.npz"))
    m = load_seeded(Slices3DRegModel(n_slices=12, mode="train", prec=prec), 0).cuda()
    m.train()
    m.train_dropout = 0.0
    batch = {k: torch.from_numpy(z[k]).cuda() for k in
             ("img_input", "img_slices", "qry_norot", "sdf", "obj_rot_mat", "trans_mat_wo_rot_tp")}
    out = m(batch)
    assert out["sdf_pred"].requires_grad and out["slices_rec"].shape == (2, 36, 32, 32)
    lp, li, lv = _reference_style_losses(out, batch)
    (lp + li + lv).backward()
    want = z["losses"]
    assert np.abs(out["sdf_pred"].detach().cpu().numpy() - z["sdf_pred"]).max() < 1e-4
    for got, w in zip((lp, li, lv), want[:3]):
        assert abs(float(got) - w) < 2e-5 * abs(w) + 1e-7, (float(got), w)
    grads = {k: p.grad.reshape(-1).cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}
    assert set(grads) == {str(k) for k in z["grad_names"]}         # exactly the tensors the reference gives a gradient
    from helpers import check_grads_against_golden
    worst = check_grads_against_golden(z, grads, skip=PRE_BN_BIASES)
    for key in z.files:
        if key.startswith("bn:") and ".down5_." not in key:
            assert np.abs(m.state_dict()[key[3:]].cpu().numpy() - z[key]).max() < 1e-5, key
    print("autograd path (%s): worst sampled-gradient error / max|g| = %.2e" % (prec, worst))


def test_autograd_path_equals_fused_step_and_trains_with_torch_adam():
    """(1) custom loss weights flow through: gradients of 2*L1(sdf) + 0.5*L1(img) + 3*vgg from the autograd path equal
    the fused step's gradient pieces recombined; (2) a plain reference-style loop with torch.optim.Adam reduces the
    loss; (3) gradients accumulate across two backward calls like any torch gradient."""
    from slice3d_amd.models import Slices3DRegModel
    from slice3d_amd.synth import make_feed_dict
    from slice3d_amd.weights import load_seeded
    batch = {k: v.cuda() for k, v in make_feed_dict(2, 32, 300, 12, seed=8).items()}
    m = load_seeded(Slices3DRegModel(n_slices=12, mode="train"), 0).cuda().train()
    m.train_dropout = 0.0
    out = m(batch)
    lp, li, lv = _reference_style_losses(out, batch)
    (lp + li + lv).backward()
    g1 = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    m2, tr = make_trainer(12)
    tr.forward_backward(batch)
    for k, p in zip(tr.names, tr.params):
        if k in PRE_BN_BIASES:
            continue
        a, b = g1[k], p.grad
        assert float((a - b).norm()) <= 1e-4 * float(b.norm()) + 1e-9, k
    # second backward without zero_grad: accumulation; weighted loss: linearity in the output gradients
    out = m(batch)
    lp, li, lv = _reference_style_losses(out, batch)
    (lp + li + lv).backward()
    for k, p in m.named_parameters():
        if p.grad is not None and k not in PRE_BN_BIASES:
            assert float((p.grad - 2 * g1[k]).norm()) <= 1e-4 * float(g1[k].norm()) + 1e-8, k
    opt = torch.optim.Adam(m.parameters(), lr=3e-4)                     # train.py:136
    first = last = None
    for it in range(12):
        opt.zero_grad()
        out = m(batch)
        loss = sum(_reference_style_losses(out, batch))
        loss.backward()
        opt.step()
        first = float(loss) if first is None else first
        last = float(loss)
    assert last < 0.85 * first, (first, last)
    with torch.no_grad():
        assert torch.isfinite(m.eval()(batch)["sdf_pred"]).all()


def test_shard_gradients_match_ddp_golden():
    """SURVEY.md 8(e) parity oracle: the HIP step on each one-sample shard reproduces the reference's per-shard
    gradients (g6 goldens: full small tensors + sampled entries of the mean), and the mean over shards is what the
    all-reduce must deliver (the exchange itself is covered on CPU with the same payload, tests/test_parallel_cpu.py)."""
    from helpers import check_grads_against_golden
    z = np.load(os.path.join(GOLDEN, "g6_ddp_shards_s32_n12_q160_b2.npz"))
    keys = ("img_input", "img_slices", "qry_norot", "sdf", "obj_rot_mat", "trans_mat_wo_rot_tp")
    full = [str(k) for k in z["full_names"]]
    shard = []
    for r in range(2):
        m, tr = make_trainer(12)
        tr.forward_backward({k: torch.from_numpy(z[k][r:r + 1]).cuda() for k in keys})
        shard.append(tr.grad_flat.cpu().clone())
        named = dict(m.named_parameters())
        for k in full:
            if k in PRE_BN_BIASES:
                continue
            g, want = named[k].grad.cpu().numpy(), z["g%d:%s" % (r, k)]
            assert np.linalg.norm(g - want) <= 2e-2 * np.linalg.norm(want) + 1e-7, (r, k)
    mean = (shard[0] + shard[1]) / 2
    grads = {k: mean[tr.offsets[k]:tr.offsets[k] + p.numel()].numpy() for k, p in zip(tr.names, tr.params)}
    assert set(grads) == {str(k) for k in z["grad_names"]}
    check_grads_against_golden(z, grads, skip=PRE_BN_BIASES)


_smooth_oracle = {}
GATE_FREE = ("att_decoder.layers.2.linear2.", "att_decoder.layers.2.norm2.", "fc_out.")


def _smooth_output_grads(b, s, q, ns, seed):
    """Fixed output gradients with no sign(.) in them: seeded normals of the size the L1 losses hand out."""
    g = torch.Generator().manual_seed(seed)
    w_sdf = torch.randn(b, q, generator=g) / (b * q)
    w_rec = torch.randn(b, 3 * ns, s, s, generator=g) / (b * 3 * ns * s * s)
    return w_sdf, w_rec, 1.0


def _oracle_smooth_grads(fd, ns, w_sdf, w_rec, w_vgg, dtype):
    from oracle import ref_cpu
    sd = seeded_sd_from_shapes(_shapes(ns), dtype=dtype)
    for k, v in sd.items():
        if v.is_floating_point() and "running" not in k and not k.startswith("vggptlossfunc"):
            v.requires_grad_(True)
    f = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in fd.items()}
    _, _, out, _ = ref_cpu.forward_train(sd, f, ns, 0.0)
    ((out["sdf_pred"] * w_sdf.to(dtype)).sum() + (out["slices_rec"] * w_rec.to(dtype)).sum() + w_vgg * out["vgg_loss"]).backward()
    return out["sdf_pred"].detach(), {k: v.grad for k, v in sd.items() if v.grad is not None}


def _smooth_case_oracle(b, s, q, ns):
    """Compact oracle outputs (sdf_pred in fp32, sampled fp32 / fp64 gradients) of one smooth-gradient case: the committed
    golden tests/golden/oracle_smooth_b<b>_s<s>_q<q>_n<ns>.npz when there is one (the 128^2 x 16 384 case; written by
    tests/golden/make_oracle_golden.py from this function), else computed here (the small case: the family's live oracle)."""
    from helpers import compact_grads, load_oracle_golden
    from slice3d_amd.synth import make_feed_dict
    key = (b, s, q, ns)
    if key not in _smooth_oracle:
        z = load_oracle_golden("smooth_b%d_s%d_q%d_n%d" % key)
        if z is None:
            fd = make_feed_dict(b, s, q, ns, seed=4000 + q)
            w_sdf, w_rec, w_vgg = _smooth_output_grads(b, s, q, ns, seed=q)
            sdf32, g32 = _oracle_smooth_grads(fd, ns, w_sdf, w_rec, w_vgg, torch.float32)
            _, g64 = _oracle_smooth_grads(fd, ns, w_sdf, w_rec, w_vgg, torch.float64)
            z = compact_grads(g32, g64)
            z["sdf_pred"] = sdf32.numpy()
        _smooth_oracle[key] = z
    return _smooth_oracle[key]


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("b,s,q,ns", [(2, 32, 128, 12), (1, 128, 16384, 12)])
def test_smooth_output_gradients_sit_at_the_fp32_floor_of_the_reference(b, s, q, ns, prec):
    """Gradient parity WITHOUT the L1 losses' sign noise: the same fixed, smooth output gradients (seeded normals on
    sdf_pred and slices_rec, 1 on vgg_loss) are pushed through the autograd path of the HIP model (s3d_train_fwd /
    s3d_train_bwd behind _TrainForward) and through CPU autograd of the oracle, dropout 0.

    What the first version of this test found: the ORACLE ITSELF, evaluated in fp32 and in fp64, differs by 2e-3 relative
    L2 in every tensor upstream of the first full-width ReLU (layer 1's FFN: 6.8 M hidden units at 32^2 / 128 queries, a
    handful of which have pre-activations within fp32 rounding of zero — their gates flip between two fp32 evaluations,
    each flip moves one unit's whole contribution), and by 1e-6 .. 3e-4 downstream of it.  The HIP gradients show the same
    pattern against the fp32 oracle (4e-6 in layer 2 / fc_out, 2e-3 upstream).  So the gate is stated against the exact
    gradient: per tensor  rel(hip, ref_fp64) <= 3 * max(rel(ref_fp32, ref_fp64), its median) + 3e-4, and the medians within
    a factor 1.5 — the HIP path is no farther from the fp64 gradient than an fp32 evaluation of the reference is."""
    from helpers import assert_fp64_anchored_gate, fp64_anchored_rows
    from slice3d_amd.models import Slices3DRegModel
    from slice3d_amd.synth import make_feed_dict
    from slice3d_amd.weights import load_seeded
    fd = make_feed_dict(b, s, q, ns, seed=4000 + q)
    w_sdf, w_rec, w_vgg = _smooth_output_grads(b, s, q, ns, seed=q)
    key = (b, s, q, ns)
    z = _smooth_case_oracle(b, s, q, ns)
    m = load_seeded(Slices3DRegModel(n_slices=ns, mode="train", prec=prec), 0).cuda().train()
    m.train_dropout = 0.0
    out = m({k: v.cuda() for k, v in fd.items()})
    assert (out["sdf_pred"].detach().cpu() - torch.from_numpy(z["sdf_pred"])).abs().max() < 1e-4
    ((out["sdf_pred"] * w_sdf.cuda()).sum() + (out["slices_rec"] * w_rec.cuda()).sum() + w_vgg * out["vgg_loss"]).backward()
    # pre-BN biases: exact gradient 0, rounding noise on both sides
    rows = fp64_anchored_rows(z, {k: p.grad for k, p in m.named_parameters()}, skip=PRE_BN_BIASES)
    # the tensors no ReLU gate sits behind (last layer's lin2 / norm2, fc_out): tight against the fp32 oracle itself.  (In
    # f16x3 mode the last layer's own gate already flips a unit now and then — its pre-activations are 22-bit — which
    # moves that layer's linear1 / attention gradients by 1e-3, the fp32 oracle's own distance from fp64 there is 3e-4.)
    med_hip, med_ref, worst = assert_fp64_anchored_gate(rows, GATE_FREE)
    print("smooth-gradient parity %s (%s): median rel-L2 vs fp64  hip %.2e / fp32 oracle %.2e;  worst tensor %s: hip %.2e, "
          "fp32 oracle %.2e;  tensors with no ReLU gate behind them (hip vs fp32 oracle): max %.2e"
          % (key, prec, med_hip, med_ref, worst[0], worst[1], worst[2], max(r[3] for r in rows if r[0].startswith(GATE_FREE))))


# ------------------------------------------------------------------------------------------------------------------
# BASELINE configs[1], training leg, at the size the headline number is quoted on: B = 4, 256^2, 12 slices, 100 000 queries
# ------------------------------------------------------------------------------------------------------------------
_full_oracle = {}
FULL = dict(b=4, s=256, q=100000, ns=12, n_sel=2048)


def _full_size_case():
    """Inputs, SPARSE smooth output gradients and the query subset they live on.  Queries are independent given the
    pyramid (models.py:69-84), so the oracle decodes only the selected 2 048 queries per object — its feed_dict carries that
    subset — while the HIP path runs all 5.2 M token rows; the U-Net (batch-statistic BatchNorm over all four objects) and
    the VGG19 branch run in full on both sides."""
    from slice3d_amd.synth import make_feed_dict
    b, s, q, ns, n_sel = (FULL[k] for k in ("b", "s", "q", "ns", "n_sel"))
    fd = make_feed_dict(b, s, q, ns, seed=9100)
    g = torch.Generator().manual_seed(91)
    sel = torch.stack([torch.randperm(q, generator=g)[:n_sel].sort().values for _ in range(b)])      # (b, n_sel)
    w_sel = torch.randn(b, n_sel, generator=g) / (b * n_sel)
    w_sdf = torch.zeros(b, q).scatter_(1, sel, w_sel)
    w_rec = torch.zeros(b, 3 * ns, s, s)
    w_rec[:, :, 1::4, 2::4] = torch.randn(b, 3 * ns, s // 4, s // 4, generator=g) / (b * 3 * ns * (s // 4) ** 2)
    fd_sub = dict(fd, qry_norot=torch.gather(fd["qry_norot"], 1, sel[:, :, None].expand(-1, -1, 3)).contiguous(),
                  sdf=torch.gather(fd["sdf"], 1, sel).contiguous())
    return fd, fd_sub, sel, w_sel, w_sdf, w_rec, 1.0


def _full_size_oracle(dtype):
    """(sdf on the subset, slices_rec, vgg_loss, gradients, updated BN statistics) of the oracle in `dtype`."""
    from oracle import ref_cpu
    if dtype not in _full_oracle:
        fd, fd_sub, sel, w_sel, w_sdf, w_rec, w_vgg = _full_size_case()
        nthr = torch.get_num_threads()
        torch.set_num_threads(min(64, os.cpu_count() or 8))     # ATen's CPU kernels get slower beyond ~32-64 threads
        try:
            sd = seeded_sd_from_shapes(_shapes(FULL["ns"]), dtype=dtype)
            for k, v in sd.items():
                if v.is_floating_point() and "running" not in k and not k.startswith("vggptlossfunc"):
                    v.requires_grad_(True)
            f = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in fd_sub.items()}
            _, _, out, ts = ref_cpu.forward_train(sd, f, FULL["ns"], 0.0)
            ((out["sdf_pred"] * w_sel.to(dtype)).sum() + (out["slices_rec"] * w_rec.to(dtype)).sum()
             + w_vgg * out["vgg_loss"]).backward()
            _full_oracle[dtype] = (out["sdf_pred"].detach(), out["slices_rec"].detach().float(), float(out["vgg_loss"]),
                                   {k: v.grad for k, v in sd.items() if v.grad is not None},
                                   {k: v.detach().float() for k, v in ts.new_stats.items()})
            del out, sd
        finally:
            torch.set_num_threads(nthr)
    return _full_oracle[dtype]


REC_PROBE = 5      # the committed oracle keeps slices_rec at every fifth pixel (rows and columns 1, 6, 11, ...): 0.37 M of 9.4 M values


def _full_size_oracle_compact():
    """Compact form of both oracle passes (fp32 + fp64) of the full-size step: sdf on the selected queries, slices_rec on a
    strided pixel probe + its exact L1 loss against the targets, the perceptual loss in both precisions, the updated
    BatchNorm statistics, sampled gradients (helpers.compact_grads).  Committed as tests/golden/oracle_train_full_b4_s256.npz
    by tests/golden/make_oracle_golden.py (20 min of CPU in the authoring container; the GPU box recomputed it in every
    run: 133 s); S3D_LIVE_ORACLE=1 recomputes."""
    from helpers import compact_grads, load_oracle_golden
    if "z" not in _full_oracle:
        z = load_oracle_golden("train_full_b4_s256")
        if z is None:
            fd, fd_sub, sel, w_sel, w_sdf, w_rec, w_vgg = _full_size_case()
            sdf32, rec32, vgg32, g32, bn32 = _full_size_oracle(torch.float32)
            _, _, vgg64, g64, _ = _full_size_oracle(torch.float64)
            z = compact_grads(g32, g64)
            z["sdf_sel"] = sdf32.float().numpy()
            z["rec_probe"] = rec32[:, :, 1::REC_PROBE, 1::REC_PROBE].contiguous().numpy()
            z["l_img"] = np.array([float((rec32 - fd["img_slices"]).abs().mean())])
            z["vgg"] = np.array([vgg32, vgg64])
            for k, v in bn32.items():
                z["bn:" + k] = v.numpy()
        _full_oracle["z"] = z
    return _full_oracle["z"]


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_full_size_train_step_matches_the_oracle_through_sparse_output_gradients(prec):
    """train.py:41-53 / models.py:48-94 in train mode at BASELINE configs[1]'s training shape (B = 4, 256^2 x 12 slices,
    Q = 100 000: 5.2 M token rows — the grid / chunking / 64-bit index paths of every training kernel that the smaller
    parity shapes never reach), dropout 0, batch-statistic BatchNorm, through the autograd form of the step.
    Checked against the oracle (fp32 and fp64; committed compact outputs, see _full_size_oracle_compact): sdf_pred on the
    4 x 2 048 selected queries and slices_rec (every fifth pixel) < 1e-4, the image and perceptual losses, the updated
    BatchNorm running statistics, and every parameter gradient by the fp64-anchored gate of the smooth-gradient test above
    (no farther from the exact gradient than 3x the fp32 oracle), over the sampled entries."""
    import time
    from helpers import assert_fp64_anchored_gate, fp64_anchored_rows
    from slice3d_amd.models import Slices3DRegModel
    from slice3d_amd.weights import load_seeded
    fd, fd_sub, sel, w_sel, w_sdf, w_rec, w_vgg = _full_size_case()
    t0 = time.time()
    z = _full_size_oracle_compact()
    t_oracle = time.time() - t0
    sdf32, rec32p = torch.from_numpy(z["sdf_sel"]), torch.from_numpy(z["rec_probe"])
    vgg32, vgg64 = (float(v) for v in z["vgg"])
    m = load_seeded(Slices3DRegModel(img_size=FULL["s"], n_slices=FULL["ns"], mode="train", prec=prec), 0).cuda().train()
    m.train_dropout = 0.0
    out = m({k: v.cuda() for k, v in fd.items()})
    sdf = out["sdf_pred"].detach().cpu()
    assert sdf.shape == (FULL["b"], FULL["q"]) and torch.isfinite(sdf).all()
    e_sdf = float((torch.gather(sdf, 1, sel) - sdf32).abs().max())
    rec = out["slices_rec"].detach().cpu()
    assert torch.isfinite(rec).all()
    e_rec = float((rec[:, :, 1::REC_PROBE, 1::REC_PROBE] - rec32p).abs().max())
    assert e_sdf < 1e-4 and e_rec < 1e-4, (e_sdf, e_rec)
    # the three losses of train.py:29-47 from these outputs (the sdf loss on the subset the oracle decodes)
    l_sdf = float((torch.gather(sdf, 1, sel) - fd_sub["sdf"]).abs().mean())
    l_sdf_ref = float((sdf32 - fd_sub["sdf"]).abs().mean())
    l_img, l_img_ref = float((rec - fd["img_slices"]).abs().mean()), float(z["l_img"][0])    # over ALL pixels on both sides
    assert abs(l_sdf - l_sdf_ref) < 2e-5 * l_sdf_ref and abs(l_img - l_img_ref) < 2e-5 * l_img_ref
    assert abs(float(out["vgg_loss"]) - vgg64) < 5e-5 * abs(vgg64), (float(out["vgg_loss"]), vgg32, vgg64)
    ((out["sdf_pred"] * w_sdf.cuda()).sum() + (out["slices_rec"] * w_rec.cuda()).sum() + w_vgg * out["vgg_loss"]).backward()
    torch.cuda.synchronize()
    sd_now = m.state_dict()
    n_bn = 0
    for k in z:
        if not k.startswith("bn:") or ".down5_." in k:
            continue
        v = torch.from_numpy(z[k])
        assert float((sd_now[k[3:]].cpu() - v).abs().max()) < 1e-5 * max(1.0, float(v.abs().max())), k
        n_bn += 1
    assert n_bn >= 40
    rows = fp64_anchored_rows(z, {k: p.grad for k, p in m.named_parameters()}, skip=PRE_BN_BIASES)
    med_hip, med_ref, worst = assert_fp64_anchored_gate(rows, GATE_FREE)
    print("full-size train (%s): sdf %.2e, rec %.2e; gradients vs fp64: median hip %.2e / fp32 oracle %.2e; worst %s: hip %.2e, "
          "fp32 oracle %.2e; gate-free tensors vs fp32 oracle: max %.2e; oracle time %.0f s"
          % (prec, e_sdf, e_rec, med_hip, med_ref, worst[0], worst[1], worst[2],
             max(r[3] for r in rows if r[0].startswith(GATE_FREE)), t_oracle))


@pytest.mark.timeout(900)
def test_full_size_fused_train_step_is_finite_and_repeatable():
    """The fused step (s3d_train_fwd_bwd, the form bench.py times) at the same full size with DENSE loss gradients and the
    reference's dropout 0.1: every loss and gradient finite; two runs with the same seed give BIT-IDENTICAL losses and gradients for
    every parameter (round 6: the sampling backward, the step's last float-atomic summation, is the atomic-free train_sbd.hip —
    fixed-order sums per tile, per-tile slots added in ascending tile order)."""
    from slice3d_amd.models import Slices3DRegModel
    from slice3d_amd.synth import make_feed_dict
    from slice3d_amd.trainer import HipTrainer
    from slice3d_amd.weights import load_seeded
    b, s, q, ns = (FULL[k] for k in ("b", "s", "q", "ns"))
    batch = {k: v.cuda() for k, v in make_feed_dict(b, s, q, ns, seed=9100).items()}
    import gc
    gc.collect()
    torch.cuda.empty_cache()          # the step's workspace is 108 GB at this size: one trainer, the earlier tests' freed
    m = load_seeded(Slices3DRegModel(img_size=s, n_slices=ns, mode="train"), 0).cuda()
    tr = HipTrainer(m, prec="f16x3", dropout=0.1, seed=11)
    stats0 = {k: v.clone() for k, v in m.state_dict().items() if "running" in k}
    runs = []
    for _ in range(2):
        tr._calls = 0                 # the same dropout seed for both runs
        m.load_state_dict(stats0, strict=False)      # the step moves the BatchNorm running statistics
        losses = tr.forward_backward(batch).cpu()
        torch.cuda.synchronize()
        assert torch.isfinite(losses).all() and torch.isfinite(tr.grad_flat).all()
        runs.append((losses.clone(), tr.grad_flat.clone()))
    (l0, g0), (l1, g1) = runs
    assert torch.equal(l0, l1)
    for k, p in zip(tr.names, tr.params):
        off, n = tr.offsets[k], p.numel()
        a, c = g0[off:off + n], g1[off:off + n]
        assert float(a.abs().max()) > 0 or k in PRE_BN_BIASES, k
        assert torch.equal(a, c), k
    print("full-size fused step: losses %s; every gradient bit-identical run to run" % (l0.tolist(),))


@pytest.mark.parametrize("prec,size,nq", [("f32", 64, 8192), ("f16x3", 64, 8192), ("f16x3", 128, 6000), ("f32", 96, 4200), ("f16x3", 32, 5000)])
def test_atomic_free_sampling_backward_matches_the_atomic_kernels(prec, size, nq, monkeypatch):
    """train_sbd.hip against the kernels it replaces (S3D_SBD_OFF=1: sample_bwd_tiled_kernel, LDS + global float atomics) on the same
    step: every gradient within fp32 summation-order noise; and with every fifth sorted slot forced through the new kernel's
    out-of-footprint path (S3D_SBD_SLOW_MOD=5: that query's row added to the maps directly) the same again.  Sizes 32 ... 128 (96: not a
    power of two) walk the footprint geometry of sbd_geom / sbd_reduce_kernel; the full size is the repeatability test above."""
    from slice3d_amd.models import Slices3DRegModel
    from slice3d_amd.synth import make_feed_dict
    from slice3d_amd.trainer import HipTrainer
    from slice3d_amd.weights import load_seeded
    ns = 12 if size <= 64 else 5
    fd = make_feed_dict(2, size, nq, ns, seed=5, device="cuda")
    m = load_seeded(Slices3DRegModel(img_size=size, n_slices=ns, mode="train"), 0).cuda()
    tr = HipTrainer(m, prec=prec, dropout=0.0, seed=3)
    stats0 = {k: v.clone() for k, v in m.state_dict().items() if "running" in k}
    grads = {}
    for mode, env in (("atomic", {"S3D_SBD_OFF": "1"}), ("dense", {}), ("dense2", {}), ("slow", {"S3D_SBD_SLOW_MOD": "5"})):
        for k in ("S3D_SBD_OFF", "S3D_SBD_SLOW_MOD"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        tr._calls = 0
        m.load_state_dict(stats0, strict=False)
        tr.forward_backward(fd)
        torch.cuda.synchronize()
        grads[mode] = tr.grad_flat.clone()
    assert torch.equal(grads["dense"], grads["dense2"])
    gmax = max(float(grads["atomic"][tr.offsets[k]:tr.offsets[k] + p.numel()].norm()) for k, p in zip(tr.names, tr.params))
    for mode in ("dense", "slow"):
        for k, p in zip(tr.names, tr.params):
            if k in PRE_BN_BIASES:
                continue
            off, n = tr.offsets[k], p.numel()
            a, c = grads["atomic"][off:off + n], grads[mode][off:off + n]
            assert float((a - c).norm()) < 2e-5 * float(a.norm()) + 1e-7 * gmax, (mode, k)


def test_single_pass_f16_training_mode_tracks_the_split_precision_step():
    """Round 6: `HipTrainer(prec="f16")` = S3D_PREC_F16 of s3d_train_fwd_bwd, the THROUGHPUT mode of the training step (the decoder's
    GEMM kernels run one f16 MFMA per product; the 13 x 13 attention core backward, the U-Net, VGG, samplers, reductions, fp32 master
    weights and the backward scale are the split-precision path's).  Not fp32-class and never the reported train_samples_per_s —
    this test pins what it is: from identical weights, batch and dropout masks the forward outputs agree to 2e-2, the losses to
    1e-2 relative, every parameter gradient (pre-BatchNorm biases aside) to 5e-2 relative L2 with a median below 1e-2, everything
    finite; and twenty Adam steps of both modes from the same start end with the same loss to 10 %."""
    from slice3d_amd.models import Slices3DRegModel
    from slice3d_amd.synth import make_feed_dict
    from slice3d_amd.trainer import HipTrainer
    from slice3d_amd.weights import load_seeded
    fd = make_feed_dict(2, 64, 8192, 12, seed=17, device="cuda")
    res = {}
    for prec in ("f16x3", "f16"):
        m = load_seeded(Slices3DRegModel(img_size=64, n_slices=12, mode="train"), 0).cuda()
        tr = HipTrainer(m, dropout=0.1, seed=11, prec=prec)
        losses, sdf, rec = tr.forward_backward(fd, want_outputs=True)
        res[prec] = (losses.cpu().numpy().copy(), sdf.clone(), rec.clone(),
                     {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None})
    l3, s3, r3, g3 = res["f16x3"]
    l1, s1, r1, g1 = res["f16"]
    assert torch.isfinite(s1).all() and all(torch.isfinite(v).all() for v in g1.values())
    assert (s1 - s3).abs().max() < 2e-2 and torch.equal(r1, r3)      # the U-Net is the split-precision path in both modes
    for i in range(3):
        assert abs(l1[i] - l3[i]) < 1e-2 * abs(l3[i]) + 1e-6, (i, l1, l3)
    dev = sorted((float((g1[k] - g).norm() / g.norm()), k) for k, g in g3.items() if k not in PRE_BN_BIASES and float(g.norm()) > 0)
    assert len(dev) > 120 and dev[-1][0] < 5e-2 and dev[len(dev) // 2][0] < 1e-2, (dev[-3:], dev[len(dev) // 2])
    end = {}
    for prec in ("f16x3", "f16"):
        m = load_seeded(Slices3DRegModel(img_size=64, n_slices=12, mode="train"), 0).cuda()
        tr = HipTrainer(m, dropout=0.1, seed=3, prec=prec)
        for _ in range(20):
            lp = tr.train_step(fd)[0]
        end[prec] = lp
    assert end["f16"] == end["f16"] and abs(end["f16"] - end["f16x3"]) < 0.1 * abs(end["f16x3"]), end
    print("single-pass f16 training mode: worst gradient deviation %.2e (%s), median %.2e; loss_pred after 20 steps %.4f vs %.4f"
          % (dev[-1][0], dev[-1][1], dev[len(dev) // 2][0], end["f16"], end["f16x3"]))


def test_train_entry_points_reject_bad_arguments():
    """The argument checks that open s3d_train_fwd_bwd, s3d_train_fwd, s3d_train_bwd and s3d_gt_train_fwd_bwd, through raw ctypes
    calls with one fault at a time on otherwise valid arguments: a NULL parameter struct, a size that is no multiple of 16, dropout
    1.0 and an unknown precision are S3D_E_ARG, a workspace one byte short is S3D_E_WORKSPACE; so are a NULL output of the forward
    half and a NULL slices_rec of the backward half.  Every case returns before anything is launched."""
    import ctypes as C
    from slice3d_amd import _lib
    from slice3d_amd.models import data_ptr, vgg_params
    from slice3d_amd.models_gt import Slices3DGTModel
    from slice3d_amd.synth import make_feed_dict
    from slice3d_amd.trainer import HipGtTrainer
    from slice3d_amd.weights import load_seeded
    E_ARG, E_WS = -1, -2
    b, s, q, ns = 1, 32, 16, 12
    fd = make_feed_dict(b, s, q, ns, seed=1, device="cuda")
    m, tr = make_trainer(ns)
    mg = load_seeded(Slices3DGTModel(n_slices=ns, mode="train"), 0).cuda()
    tg = HipGtTrainer(mg)
    lib, dev = tr.lib, tr.grad_flat.device
    st = _lib.stream_ptr(dev)
    (u, h), v = tr._structs(data_ptr), vgg_params(m, data_ptr)
    du, dh = tr._structs(tr._gptr)
    ge, gh = tg._structs(data_ptr)
    dge, dgh = tg._structs(tg._gptr)
    tb = tr._batch_struct(tr._batch(fd, ("img_input", "img_slices", "qry_norot", "obj_rot_mat", "trans_mat_wo_rot_tp", "sdf")))
    need = {"reg": lib.s3d_train_workspace_bytes(b, s, q, ns), "gt": lib.s3d_gt_train_workspace_bytes(b, s, q, ns)}
    # large enough for S = 40 too, so that no call can be refused for its workspace before its size is looked at
    nws = max(max(need.values()), lib.s3d_train_workspace_bytes(b, 40, q, ns), lib.s3d_gt_train_workspace_bytes(b, 40, q, ns))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    losses = torch.zeros(4, device=dev)
    vgg = torch.zeros((), device=dev)
    sdf = torch.zeros(b, q, device=dev)
    rec = torch.zeros(b * ns, 3, s, s, device=dev)
    P = lambda x: C.byref(x)

    def fused(U=P(u), S=s, p=0.1, prec=_lib.PREC_F32, n=nws):
        return lib.s3d_train_fwd_bwd(U, P(h), P(v), P(du), P(dh), P(tb), b, S, q, ns, p, 1, prec, losses.data_ptr(),
                                     sdf.data_ptr(), rec.data_ptr(), ws.data_ptr(), n, st)

    def fwd(U=P(u), S=s, p=0.1, prec=_lib.PREC_F32, n=nws, out=sdf.data_ptr()):
        return lib.s3d_train_fwd(U, P(h), P(v), P(tb), b, S, q, ns, p, 1, prec, vgg.data_ptr(), out, rec.data_ptr(),
                                 ws.data_ptr(), n, st)

    def bwd(U=P(u), S=s, p=0.1, prec=_lib.PREC_F32, n=nws, slices_rec=rec.data_ptr()):
        return lib.s3d_train_bwd(U, P(h), P(v), P(du), P(dh), P(tb), b, S, q, ns, p, 1, prec, sdf.data_ptr(), None, 0.0, 0.0,
                                 slices_rec, ws.data_ptr(), n, st)

    def gt(U=P(ge), S=s, p=0.1, prec=_lib.PREC_F32, n=nws):
        return lib.s3d_gt_train_fwd_bwd(U, P(gh), P(dge), P(dgh), P(tb), b, S, q, ns, p, 1, prec, losses.data_ptr(),
                                        sdf.data_ptr(), ws.data_ptr(), n, st)

    for name, call, size in (("s3d_train_fwd_bwd", fused, need["reg"]), ("s3d_train_fwd", fwd, need["reg"]),
                             ("s3d_train_bwd", bwd, need["reg"]), ("s3d_gt_train_fwd_bwd", gt, need["gt"])):
        assert call(U=None) == E_ARG and b"null" in lib.s3d_last_error().lower(), name
        assert call(S=40) == E_ARG, name
        assert call(p=1.0) == E_ARG, name
        assert call(prec=7) == E_ARG, name
        assert call(n=size - 1) == E_WS, name
    assert fwd(out=None) == E_ARG
    assert bwd(slices_rec=None) == E_ARG
    torch.cuda.synchronize()
    assert float(losses.abs().sum()) == 0.0      # nothing ran
