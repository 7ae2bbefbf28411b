"""Formula-generated inputs shared by tests/golden/make_golden_gen_route.py and tests/test_gen_route.py: integer
arithmetic and single correctly rounded fp32 operations only, so both sides rebuild the same bits on any machine."""
import hashlib

import numpy as np
import torch
from PIL import Image

SIZE = 128
TOY_SHAPES = ("obj_a", "obj_b", "obj_c")


def sample_tensor(b, c, s=SIZE, seed=0):
    """(b, c, s, s) float32 'decoded tiles': a ramp over [-1.2, 1.2] with, at every 7th element, a truncation boundary
    (2k - 255) / 255 of the * 255 quantisation or one of its fp32 neighbours, and runs of exactly +1 and -1."""
    i = np.arange(b * c * s * s, dtype=np.int64)
    h = (i * 2654435761 + seed * 97) % 6007
    v = (h - 3003).astype(np.float32) / np.float32(2500)
    k = (i // 7) % 256
    bnd = (2 * k - 255).astype(np.float32) / np.float32(255)
    near = np.where(i % 3 == 0, np.nextafter(bnd, np.float32(-2)),
                    np.where(i % 3 == 1, bnd, np.nextafter(bnd, np.float32(2)))).astype(np.float32)
    v = np.where(i % 7 == 0, near, v).astype(np.float32)
    v[1::1009] = 1.0
    v[5::1009] = -1.0
    return torch.from_numpy(v.reshape(b, c, s, s))


def input_views(b, s=SIZE, seed=0):
    """(b, s, s, 3) img_ipt_view entries as ObjaverseBase makes them: u8 / 127.5 - 1 (float64, then float32), every u8."""
    i = np.arange(b * s * s * 3, dtype=np.int64)
    u8 = ((i * 31 + seed) % 256).astype(np.uint8).reshape(b, s, s, 3)
    return torch.from_numpy((u8 / 127.5 - 1.0).astype(np.float32))


def mosaic_u8(idx, s=SIZE):
    """A (4s, 4s, 3) uint8 mosaic whose every tile differs from the others and from every other mosaic."""
    y, x, ch = np.meshgrid(np.arange(4 * s), np.arange(4 * s), np.arange(3), indexing="ij")
    return ((x * 3 + y * 5 + ch * 7 + idx * 11 + (y // s) * 4 * 13 + (x // s) * 13) % 256).astype(np.uint8)


def rgba_object(w=96, h=80):
    """An RGBA image with an opaque ellipse off the centre (for create_dataset_sin_img.py's centring)."""
    y, x = np.mgrid[0:h, 0:w]
    a = (((x - 25) / 14.0) ** 2 + ((y - 55) / 9.0) ** 2 <= 1).astype(np.uint8) * 255
    rgb = np.stack([(x * 2) % 256, (y * 3) % 256, (x + y) % 256], -1).astype(np.uint8)
    return Image.fromarray(np.concatenate([rgb, a[..., None]], -1), "RGBA")


def pixel_sha(path):
    """SHA-256 of a PNG's decoded pixels, with its mode and size."""
    im = Image.open(path)
    return "%s:%dx%d:%s" % (im.mode, im.size[0], im.size[1], hashlib.sha256(np.asarray(im).tobytes()).hexdigest())


def array_sha(a):
    a = np.ascontiguousarray(a)
    return "%s:%s:%s" % (a.dtype.str, "x".join(map(str, a.shape)), hashlib.sha256(a.tobytes()).hexdigest())


def tree_digest(root):
    """{relative path: pixel_sha (png) | array_sha (npy) | 'bytes:' + sha (other)} of every file under root."""
    import os
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            rel = os.path.relpath(p, root).replace(os.sep, "/")
            if f.endswith(".png"):
                out[rel] = pixel_sha(p)
            elif f.endswith(".npy"):
                out[rel] = array_sha(np.load(p))
            elif f.endswith(".pkl"):
                out[rel] = "pkl"
            else:
                out[rel] = "bytes:" + hashlib.sha256(open(p, "rb").read()).hexdigest()
    return out


def write_trainval(base, shapes, trailing_newline):
    import os
    with open(os.path.join(base, "03_splits", "trainval.lst"), "w") as f:
        f.write("\n".join(shapes) + ("\n" if trailing_newline else ""))
