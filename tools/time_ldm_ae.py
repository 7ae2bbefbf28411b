"""Times the gen_slices first stage and the image -> slices route on the GPU (device events after a warm-up, seeded weights):
AutoencoderKL.decode of one object's 12 tiles, the condition-plus-encode step, the wide attention primitive, and
SliceDiffusion.generate() at B = 1 and B = 4 with 200 DDIM steps.

    python tools/time_ldm_ae.py [prec]          (prec: f16x3, the default, or f32)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from slice3d_amd import _lib  # noqa: E402
from slice3d_amd.ldm_autoencoder import KL_F8, AutoencoderKL, ImageEncoderVGG16BN  # noqa: E402
from slice3d_amd.ldm_pipeline import UNET_CFG, SliceDiffusion  # noqa: E402
from slice3d_amd.ldm_unet import UNetModel  # noqa: E402
from slice3d_amd.weights import load_seeded  # noqa: E402

PREC = sys.argv[1] if len(sys.argv) > 1 else "f16x3"


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


m = SliceDiffusion(load_seeded(UNetModel(prec=PREC, **UNET_CFG), 0), load_seeded(AutoencoderKL(KL_F8, 4, prec=PREC), 0),
                   load_seeded(ImageEncoderVGG16BN(prec=PREC), 0), 0.18215).cuda().eval()
g = torch.Generator(device="cuda").manual_seed(0)
mosaic = torch.randn((1, 4, 64, 64), device="cuda", generator=g)
print("prec %s" % PREC)
print("AutoencoderKL.decode, 12 tiles of 128^2 (one object): %.2f ms" % timed(lambda: m.first_stage.decode(mosaic, n_tiles=12), 10))
for b in (1, 4):
    img = torch.rand((b, 3, 128, 128), device="cuda", generator=g) * 2 - 1
    print("condition (VGG16-BN taps + trans*) + encode + posterior sample, B=%d: %.2f ms" % (b, timed(lambda: m.condition(img), 10)))
    print("  of which AutoencoderKL.encode: %.2f ms, ImageEncoderVGG16BN: %.2f ms"
          % (timed(lambda: m.first_stage.encode(img), 10), timed(lambda: m.cond_stage(img), 10)))
lib, st = _lib.load(), _lib.stream_ptr(torch.device("cuda"))
for n, t in ((12, 256), (1, 4096)):
    qkv = torch.randn((n, t, 1536), device="cuda", generator=g)
    out = torch.empty((n, t, 512), device="cuda")
    ms = timed(lambda: lib.s3d_wide_attention_fwd(qkv.data_ptr(), out.data_ptr(), n, t, 512, _lib.PREC[PREC], st), 10)
    print("s3d_wide_attention_fwd C=512 N=%d T=%d: %.3f ms (%.1f TFLOP/s at 4 N T^2 C)" % (n, t, ms, 4 * n * t * t * 512 / ms / 1e9))
for b in (1, 4):
    img = torch.rand((b, 3, 128, 128), device="cuda", generator=g) * 2 - 1
    ms = timed(lambda: m.generate(img, ddim_steps=200, generator=g), 2, warm=1)
    print("SliceDiffusion.generate B=%d, 200 DDIM steps: %.1f ms (%.1f ms per object)" % (b, ms, ms / b))
