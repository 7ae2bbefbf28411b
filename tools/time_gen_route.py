"""Times the generation-based slicing route at the reference's test batch of 8 (device events after a warm-up, seeded
weights): SliceDiffusion.generate() with 200 DDIM steps, the autoencoder pass over 8 x 13 tiles of reconstruct_slices_ae.py,
and the in-memory image -> slices -> mesh route of reconstruct.py --gen_ckpt per object (B = 1, 200 steps, quantisation,
Slices3DGTModel + Generator3D at --mc_res0 64 --mc_up_steps 2; wall clock, mesh export excluded).

    python tools/time_gen_route.py
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from slice3d_amd import gen_route  # noqa: E402
from slice3d_amd.generator import Generator3D  # noqa: E402
from slice3d_amd.models_gt import Slices3DGTModel  # noqa: E402
from slice3d_amd.synth import make_feed_dict  # noqa: E402
from slice3d_amd.weights import load_seeded  # noqa: E402


def timed(fn, reps, warm=1):
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


m = gen_route.synthetic_slice_diffusion(0).cuda().eval()
g = torch.Generator(device="cuda").manual_seed(0)
img8 = torch.rand((8, 3, 128, 128), device="cuda", generator=g) * 2 - 1
ms = timed(lambda: m.generate(img8, ddim_steps=200, generator=g), 2)
print("SliceDiffusion.generate B=8, 200 DDIM steps: %.1f ms (%.1f ms per object)" % (ms, ms / 8))
stacks = torch.rand((8, 128, 128, 39), device="cuda", generator=g) * 2 - 1
ms = timed(lambda: gen_route.autoencode_stacks(m.first_stage, stacks, generator=g), 5)
print("autoencoder pass, 8 x 13 tiles of 128^2 (encode + posterior sample + decode): %.1f ms" % ms)

gt = load_seeded(Slices3DGTModel(img_size=128, n_slices=12, mode="test"), 0).cuda().eval()
gen = Generator3D(gt, threshold=0.5, resolution0=64, upsampling_steps=2, chunk_size=3000, pred_type="sdf")
fd = {k: v.cuda() for k, v in make_feed_dict(1, 128, 16, 12, seed=1, with_slices=False).items()}


def image_to_mesh():
    slices = m.generate(img8[:1], ddim_steps=200, generator=g)
    data = dict(fd, img_slices=gen_route.gen_slices_to_model_input(gen_route.slices_to_mosaic_u8(slices)))
    mesh = gen.generate_mesh(data, return_stats=False)
    torch.cuda.synchronize()
    return mesh


image_to_mesh()
t0 = time.perf_counter()
for _ in range(3):
    mesh = image_to_mesh()
print("image -> slices -> mesh, one object (B=1, 200 steps, MISE 64 + 2 up-steps): %.1f ms (%d verts)"
      % ((time.perf_counter() - t0) / 3 * 1e3, len(mesh.vertices)))
