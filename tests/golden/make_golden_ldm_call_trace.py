"""Fixture of tests/test_gpu_ldm_call_trace.py: the library calls of the latent-diffusion models, case by case (the cases, the
recorder and the reduction of the arguments are that module's; LDM_SMALL at batch 2 as it stands meets the test's conditions on
the fixture).  The file pins what the models did BEFORE a change of their host code, so it is written from the parent commit's
slice3d_amd/ldm_unet.py and ldm_autoencoder.py, given as a directory, and never from the code under test.  GPU box only:

    git show dbad04d:slice3d_amd/ldm_unet.py > /tmp/parent/ldm_unet.py       (likewise ldm_autoencoder.py)
    python tests/golden/make_golden_ldm_call_trace.py /tmp/parent

dbad04d is the last commit before slice3d_amd/ldm_ops.py existed; the committed fixture was recorded from it.
"""
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from test_gpu_ldm_call_trace import FIXTURE, run_cases  # noqa: E402


def load_models(src_dir):
    """(UNetModel, AutoencoderKL, ImageEncoderVGG16BN) of the ldm_unet.py / ldm_autoencoder.py in src_dir, loaded as modules
    of the slice3d_amd package beside the tree's own."""
    import slice3d_amd  # noqa: F401
    names = ["slice3d_amd.ldm_unet", "slice3d_amd.ldm_autoencoder"]
    tree = {n: sys.modules.pop(n, None) for n in names}
    try:
        for n in names:      # under the tree's names while they load: ldm_autoencoder may import .ldm_unet, and means its own
            spec = importlib.util.spec_from_file_location(n, os.path.join(src_dir, n.split(".")[1] + ".py"))
            sys.modules[n] = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(sys.modules[n])
        unet, ae = (sys.modules[n] for n in names)
    finally:
        for n in names:
            sys.modules.pop(n, None)
            if tree[n] is not None:
                sys.modules[n] = tree[n]
    return unet.UNetModel, ae.AutoencoderKL, ae.ImageEncoderVGG16BN


def write_fixture(traces, out=FIXTURE):
    """Every distinct call once, one per line, and per case the indices of its calls (the cases share most of their calls:
    load_fixture() of the test module puts the traces together again)."""
    calls, cases = {}, {}
    for case, trace in traces.items():
        cases[case] = [calls.setdefault(json.dumps(c, separators=(",", ":")), len(calls)) for c in trace]
    with open(out, "w") as fh:
        fh.write('{"calls": [\n%s\n],\n"cases": {\n%s\n}}\n' % (
            ",\n".join(calls), ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in cases.items())))
    print("wrote %s: %d distinct calls; %s" % (out, len(calls), {k: len(v) for k, v in cases.items()}))


def record(classes):
    traces = {case: json.loads(json.dumps(calls)) for case, calls, _ in run_cases(*classes)}
    torch.cuda.synchronize()
    write_fixture(traces)


if __name__ == "__main__":
    record(load_models(sys.argv[1]))
