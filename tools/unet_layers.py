"""Per-layer time and TFLOP/s of the U-Net encode (s3d_unet_encode_fwd) from a rocprofv3 kernel trace of
tools/unet_layers_run.py, against the per-layer FLOP table of BASELINE.md section 3 (256^2, 12 slices).

    rocprofv3 --kernel-trace -d /tmp/ul -o u -- python tools/unet_layers_run.py ; python tools/unet_layers.py <db> [B]
The encode launches its layers in a fixed order (api.hip: 13 encoder convs with BN+ReLU+pool after the taps, trans_c,
the latent's broadcast add, then per up stage trans_up / skip-half 3x3 (both once per image), up1's ConvT / up-half 3x3 / table kernel
(per image) or up2..up4's composed ConvT -> up-half 3x3 (one launch on the low-resolution map), and the second 3x3); a split-K layer
adds a conv_splitk_finish_kernel right after its conv."""
import sqlite3
import sys

ENC = [("conv1_1 3->64 @256", 0.23), ("conv1_2 64->64 @256", 4.83), ("conv2_1 64->128 @128", 2.42),
       ("conv2_2 128->128 @128", 4.83), ("conv3_1 128->256 @64", 2.42), ("conv3_2 256->256 @64", 4.83),
       ("conv3_3 256->256 @64", 4.83), ("conv4_1 256->512 @32", 2.42), ("conv4_2 512->512 @32", 4.83),
       ("conv4_3 512->512 @32", 4.83), ("conv5_1 512->512 @16", 1.21), ("conv5_2 512->512 @16", 1.21),
       ("conv5_3 512->512 @16", 1.21)]
TAPS = {1, 3, 6, 9}
# The decoder computes what does not depend on the slice once per image (api.hip, s3d_unet_encode_fwd): the skip 1x1 and the
# skip half of every first 3x3 (the reference runs both on the 12x expanded batch: 3.22 and 28.99 / 2 GFLOP), trans_c over
# the 512 image channels, and the whole of up1 in front of its first BatchNorm; the per-slice parts of the latter two come from
# the packed image through two elementwise kernels (0 FLOP here)
UP = []
for i, (c, r) in enumerate(((512, 32), (256, 64), (128, 128), (64, 256))):
    one = i == 0
    UP += [("up%d skip 1x1 %d->%d @%d (per image)" % (i + 1, c, c // 2, r), 3.22 / 12),
           ("up%d skip-half 3x3 %d->%d @%d (per image)" % (i + 1, c // 2, c // 2, r), 28.99 / 2 / 12)]
    if one:
        UP += [("up1 ConvT %d->%d (per image)" % (c, c // 2), 3.22 / 12),
               ("up1 up-half 3x3 %d->%d @%d + per-image term (per image)" % (c // 2, c // 2, r), 28.99 / 2 / 12),
               ("up1 + slice table, BN, ReLU -> 12 slices", 0.0)]
    else:   # K = 4 C per output pixel instead of 9 C / 2: 8 / 9 of the up-half 3x3's products, and no ConvT
        UP += [("up%d ConvT o up-half 3x3 composed, %d@%d -> %d@%d + per-image term" % (i + 1, c, r // 2, c // 2, r), 28.99 / 2 * 8 / 9)]
    UP += [("up%d 3x3 %d->%d @%d" % (i + 1, c // 2, c // 2, r), 14.50)]
LAYERS = ENC + [("trans_c 1x1 512->512 @16 (per image)", 2.01 * 512 / 640 / 12), ("latent = per image + slice vector -> 12 slices", 0.0)] + UP


def main(path, batch):
    db = sqlite3.connect(path)
    rows = db.execute("select name, start, end from kernels order by start").fetchall()
    conv_like = lambda n: ("conv3x3_lds" in n or "conv_up2x_lds" in n or "conv_igemm" in n or "lin_rows" in n or "conv3x3_first" in n or "slice_bcast_add" in n
                           or "slice_table_act" in n)
    encodes, cur = [], None
    for name, st, en in rows:
        if "conv3x3_first_kernel" in name:     # the encode's first launch
            cur = [(name, en - st)]
            encodes.append(cur)
            continue
        if cur is None:
            continue
        if conv_like(name) or "conv_splitk_finish" in name or "bn_relu_pool" in name:
            cur.append((name, en - st))
        else:
            cur = None
    acc = [[0.0, 0.0, 0.0, ""] for _ in LAYERS]      # conv us, finish us, pool us
    n_ok = 0
    for e in encodes[2:]:
        i, li, ok = 0, 0, True
        tmp = [[0.0, 0.0, 0.0, ""] for _ in LAYERS]
        while li < len(LAYERS) and i < len(e):
            name, d = e[i]
            if not conv_like(name):
                ok = False
                break
            tmp[li][0] += d / 1e3
            tmp[li][3] = name.split("(")[0].replace("void ", "")[:44]
            i += 1
            if i < len(e) and "conv_splitk_finish" in e[i][0]:
                tmp[li][1] += e[i][1] / 1e3
                i += 1
            if li in TAPS and i < len(e) and "bn_relu_pool" in e[i][0]:
                tmp[li][2] += e[i][1] / 1e3
                i += 1
            li += 1
        if ok and li == len(LAYERS):
            n_ok += 1
            for a, t in zip(acc, tmp):
                a[0] += t[0]; a[1] += t[1]; a[2] += t[2]; a[3] = t[3]
    print("# U-Net encode per layer: %d objects per call, f16x3, averaged over %d encodes (tools/unet_layers.py)\n" % (batch, n_ok))
    print("| layer | GFLOP (x%d objects) | conv us | split-K finish us | BN+ReLU+pool us | TFLOP/s algorithmic | kernel |" % batch)
    print("|---|---|---|---|---|---|---|")
    tot_f = tot_t = 0.0
    for (label, gf), a in zip(LAYERS, acc):
        us = (a[0] + a[1] + a[2]) / max(n_ok, 1)
        f = gf * batch
        tot_f += f; tot_t += us
        print("| %s | %.2f | %.1f | %.1f | %.1f | %.0f | `%s` |" % (label, f, a[0] / max(n_ok, 1), a[1] / max(n_ok, 1),
                                                                     a[2] / max(n_ok, 1), f / us * 1e3 if us else 0, a[3]))
    print("\ntotal %.1f GFLOP in %.1f us of kernel time = %.0f TFLOP/s algorithmic (x3 on the f16 pipe)" % (tot_f, tot_t, tot_f / tot_t * 1e3))


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 4)
