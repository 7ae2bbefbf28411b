"""Which kernels does the convolution engine launch?  The case table of tests/golden/conv_plan_sweep.json and its recorder.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/conv_plan_sweep.py --run --codes codes.json
    python tools/conv_plan_sweep.py --from-trace DIR/.../*_kernel_trace.csv --codes codes.json --commit <sha> --out tests/golden/conv_plan_sweep.json

--run calls s3d_conv_fwd, s3d_conv_gn_fwd (with and without nsplit_out) and s3d_conv_strided_fwd once per row of cases(),
one row after the other, with one s3d_image_normalize_fwd call in front of every row: its kernel is the row separator of the
trace.  Tensors hold zeros; the rows check the choice of kernel, not the arithmetic.  --from-trace turns the kernel trace of
such a run into the JSON: per row the arguments, the return code class (`refused`) and the ordered list of
[kernel name, grid x, grid y (workgroups), block] that ran.  tests/test_conv_plan.py holds s3d_conv_plan_describe against it.

The table: every row of tests/test_gpu_conv.py in every precision and workspace form it runs, and rows on both sides of
every decision edge of the dispatcher (conv.hip).  Edges that no shape can sit on exactly take the nearest shapes:
  * 65 pixels in maps of at most 16 pixels always exceed 160 bordered pixels (N (H+2) (W+2) >= 2.25 N H W), so the 64 | 65
    edge of the small-map 3x3 rule is taken on the 1x1 rule (its cap is 64) and the 3x3 rows take 160 | 162 bordered pixels;
  * 161 = 7 x 23 and 65 = 5 x 13 bordered pixels need maps that miss the pixel caps: 160 | 162 and 64 | 75 stand in.
"""
import argparse
import csv
import importlib.util
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32, F16X3, F16 = 0, 1, 2
SEPARATOR = "image_normalize_kernel"


def pad16(c):
    return (c + 15) // 16 * 16


def ws_floats(ws, n, h, w, cout):
    """Workspace size in floats of a row's `ws` field: none | short2 | two | big | an integer multiple of one partial."""
    of = n * h * w * pad16(cout)
    return {"none": 0, "short2": 2 * of - 1, "two": 2 * of, "big": 64 * of}[ws] if isinstance(ws, str) else ws * of


def _test_tables():
    spec = importlib.util.spec_from_file_location("_test_gpu_conv", os.path.join(ROOT, "tests", "test_gpu_conv.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.FWD_CASES, m.GN_CASES, m.STRIDED_CASES


def strided_out(hin, ks, stride, origin):
    return (hin + 1 - ks) // stride + 1 if origin else (hin + 2 * (ks // 2) - ks) // stride + 1


def cases():
    """The rows: dicts with the arguments of s3d_conv_plan_describe (workspace as `ws`, see ws_floats) plus `id`."""
    rows = []

    def fwd(rid, n, h, w, cin0, cin1, cout, ks, prec=F16X3, ws="none", gn=0, defer=0):
        rows.append(dict(id=rid, N=n, H=h, W=w, cout=cout, cin0=cin0, cin1=cin1, ks=ks, prec=prec, fused_gn=gn, ws=ws,
                         nsplit_out=defer, Hin=0, Win=0, stride=0, pad_origin=0))

    def strided(rid, n, hin, win, cin, cout, ks, stride, origin, prec=F16X3):
        rows.append(dict(id=rid, N=n, H=strided_out(hin, ks, stride, origin), W=strided_out(win, ks, stride, origin), cout=cout,
                         cin0=cin, cin1=0, ks=ks, prec=prec, fused_gn=0, ws="none", nsplit_out=0, Hin=hin, Win=win, stride=stride,
                         pad_origin=origin))

    pn = {F32: "f32", F16X3: "f16x3", F16: "f16"}
    fwd_cases, gn_cases, strided_cases = _test_tables()
    # ---- the rows of tests/test_gpu_conv.py, as that file runs them
    for name, n, h, w, cin0, cin1, cout, ks, _res, _bias, split in fwd_cases:
        for ws in (("none", "two", "big") if split else ("none",)):
            for prec in (F32, F16X3, F16):
                fwd("t:%s/%s/%s" % (name, ws, pn[prec]), n, h, w, cin0, cin1, cout, ks, prec, ws)
    for name, n, h, w, cin0, cin1, cout, _film, _silu, _res, _bias in gn_cases:
        for ws in ("none", "two", "big"):
            for prec in (F16X3, F16):
                for defer in ((0, 1) if ws != "none" else (0,)):
                    fwd("t:%s/%s/%s%s" % (name, ws, pn[prec], "/defer" if defer else ""), n, h, w, cin0, cin1, cout, 3, prec, ws, 1,
                        defer)
    for name, n, hin, win, cin, cout, ks, stride, origin in strided_cases:
        for prec in (F32, F16X3):
            strided("t:%s/%s" % (name, pn[prec]), n, hin, win, cin, cout, ks, stride, origin, prec)

    # ---- LDS-staged 3x3: the 8 x 16 tile edge (W 15 | 16, H 7 | 8), with and without a workspace, plain and fused GroupNorm
    for h, w in ((8, 16), (8, 15), (7, 16), (7, 15)):
        for ws in ("none", "big"):
            fwd("lds-edge-%dx%d/%s" % (h, w, ws), 1, h, w, 64, 0, 64, 3, ws=ws)
            fwd("lds-edge-%dx%d/%s/gn" % (h, w, ws), 1, h, w, 64, 0, 64, 3, ws=ws, gn=1)
    # workspace sizes on a tiled split-K layer: none, a float short of two partials, exactly two, large; and deferred
    for ws in ("none", "short2", "two", "big", 3):
        fwd("lds-ws/%s" % ws, 1, 9, 20, 256, 0, 64, 3, ws=ws)
        fwd("lds-ws/%s/gn-defer" % ws, 1, 9, 20, 256, 0, 64, 3, ws=ws, gn=1, defer=1)
    # workgroups per split 511 | 512 (7 x 73 | 8 x 64 tiles of a 64-channel output): split-K stops at 512
    fwd("lds-wg511", 73, 8, 112, 64, 0, 64, 3, ws=4)
    fwd("lds-wg512", 64, 8, 128, 64, 0, 64, 3, ws=4)
    fwd("lds-wg511-co32", 73, 8, 112, 64, 0, 32, 3, ws=4)
    fwd("lds-wg512-co32", 64, 8, 128, 64, 0, 32, 3, ws=4)
    # chunks per split 2 | 3 on the 32-channel tile (one buffer or two), unsplit and split; one source against two
    for cin0, cin1 in ((64, 0), (96, 0), (32, 32), (64, 32), (128, 0), (192, 0)):
        for ws in ("none", "two"):
            fwd("lds-co32-cin%d_%d/%s" % (cin0, cin1, ws), 2, 16, 32, cin0, cin1, 96, 3, ws=ws)
    fwd("lds-co64-two-sources", 2, 16, 32, 64, 32, 64, 3)
    fwd("lds-co64-two-sources/gn", 2, 16, 32, 64, 32, 64, 3, gn=1)
    fwd("lds-f16-single-pass", 2, 16, 32, 64, 0, 64, 3, prec=F16)
    fwd("lds-f32-is-menu", 2, 16, 32, 64, 0, 64, 3, prec=F32)
    # CoutPad a multiple of 16 only keeps a 3x3 off the LDS kernel; a fused GroupNorm is then refused
    fwd("lds-off-co48", 2, 16, 32, 64, 0, 48, 3)
    fwd("lds-off-co48/gn", 2, 16, 32, 64, 0, 48, 3, gn=1)
    fwd("gn-refused-cin-not-32", 2, 16, 32, 48, 0, 64, 3, gn=1)
    fwd("gn-refused-ks1", 2, 16, 32, 64, 0, 64, 1, gn=1, ws="big")
    fwd("gn-refused-f32", 2, 16, 32, 64, 0, 64, 3, prec=F32, gn=1)

    # ---- small-map 3x3 (split-K only).  (N, H, W): all-image pixels, map pixels, bordered pixels in the comment
    small3 = [
        ("p16-pt1", 1, 1, 16), ("p17-pt2", 1, 1, 17),          # PT 1 | 2
        ("p32-pt2", 2, 4, 4), ("p33-tiled", 1, 3, 11),         # the 32-pixel cap: 32 | 33
        ("hw16-p48", 3, 2, 8), ("hw17-p34", 2, 1, 17),         # H W 16 | 17 with N H W <= 64
        ("p64-hw16-b144", 4, 4, 4),                            # the 64-pixel cap of the 4 x 4 maps, PT 4
        ("b160-p64", 4, 2, 8), ("b160-p60", 5, 2, 6), ("b162-p48", 3, 1, 16),   # bordered pixels 160 | 162
        ("b64-pt1", 4, 2, 2), ("b75-pt2", 5, 1, 3), ("b144-p16-pt2", 16, 1, 1),  # one-tile form: bordered 64 | 75
    ]
    for name, n, h, w in small3:
        for ws in ("none", "short2", "two", "big"):
            fwd("small3-%s/%s" % (name, ws), n, h, w, 128, 0, 64, 3, ws=ws)
        fwd("small3-%s/big/gn" % name, n, h, w, 128, 0, 64, 3, ws="big", gn=1)
        fwd("small3-%s/big/gn-defer" % name, n, h, w, 128, 0, 64, 3, ws="big", gn=1, defer=1)
        fwd("small3-%s/none/gn" % name, n, h, w, 128, 0, 64, 3, gn=1)
    fwd("small3-co96-is-tiled", 2, 4, 4, 128, 0, 96, 3, ws="big")         # the small kernel needs 64-channel tiles
    fwd("small3-co128", 2, 4, 4, 64, 64, 128, 3, ws="big")
    fwd("small3-one-chunk-is-tiled", 2, 4, 4, 32, 0, 64, 3, ws="big")     # one chunk cannot split

    # ---- small-map 1x1 (split-K only; falls through when it would not split)
    small1 = [("p16-pt1", 1, 4, 4), ("p17-pt2", 1, 1, 17), ("p32-pt2", 2, 4, 4), ("p33-pt4", 3, 1, 11), ("p64-pt4", 1, 8, 8),
              ("p65-menu", 1, 5, 13)]
    for name, n, h, w in small1:
        for ws in ("none", "short2", "two", "big"):
            fwd("small1-%s/%s" % (name, ws), n, h, w, 128, 0, 64, 1, ws=ws)
    fwd("small1-two-sources", 2, 4, 4, 64, 64, 128, 1, ws="big")
    fwd("small1-co96-is-menu", 2, 4, 4, 128, 0, 96, 1, ws="big")          # CoutPad a multiple of 32 only
    fwd("small1-one-chunk-is-menu", 2, 4, 4, 32, 0, 64, 1, ws="big")
    fwd("small1-cin48-is-menu", 2, 4, 4, 48, 0, 64, 1, ws="big")
    fwd("small1-f32-is-menu", 2, 4, 4, 128, 0, 64, 1, prec=F32, ws="big")

    # ---- row-linear kernels: P = 65535 | 65536 (lin_rows), 131071 | 131072 (lin_stream<1>)
    for p in (65535, 65536):
        fwd("lin_rows-p%d" % p, 1, 1, p, 96, 0, 84, 1)
    for p in (131071, 131072):
        fwd("lin_stream-p%d" % p, 1, 1, p, 128, 0, 128, 1)
    fwd("lin_stream-off-cout124", 1, 1, 131072, 128, 0, 124, 1)           # cout != CoutPad keeps lin_stream off
    fwd("lin_stream-cin96-is-lin_rows", 1, 1, 131072, 96, 0, 96, 1)
    fwd("lin_rows-off-two-sources", 1, 1, 65536, 64, 32, 96, 1)
    fwd("lin_rows-off-co48", 1, 1, 65536, 96, 0, 48, 1)
    fwd("lin_rows-off-cin160", 1, 1, 65536, 160, 0, 96, 1)
    fwd("lin_rows-f16", 1, 1, 65536, 96, 0, 96, 1, prec=F16)
    fwd("lin_rows-off-f32", 1, 1, 65536, 96, 0, 96, 1, prec=F32)

    # ---- tile menu: every `want` threshold from both sides.  (cout, pixels just below the threshold); ks 1 with two sources
    # (off the row-linear kernels), ks 3 on a one-row map without a workspace (off the LDS kernel); f16 image or none (cin 16)
    menu = [(256, 255 * 128), (256, 255 * 64), (256, 127 * 32),   # CoutPad % 128: 128 x 128, 64 x 128, 32 x 128 tiles
            (192, 170 * 256), (192, 85 * 64),                     # % 64: 256 x 64, 64 x 64
            (96, 170 * 256),                                      # % 32: 256 x 32
            (48, 170 * 256)]                                      # % 16: 256 x 16
    for cout, below in menu:
        for p in (below, below + 1):
            fwd("menu-co%d-p%d-ks1-f16" % (cout, p), 1, 1, p, 32, 32, cout, 1)
            fwd("menu-co%d-p%d-ks3-f16" % (cout, p), 1, 1, p, 32, 0, cout, 3)
            fwd("menu-co%d-p%d-ks1-nof16" % (cout, p), 1, 1, p, 16, 0, cout, 1)
            fwd("menu-co%d-p%d-ks3-nof16" % (cout, p), 1, 1, p, 16, 0, cout, 3)

    # ---- s3d_conv_strided_fwd: both pad_origin values, and stride 1 (Hin = H: the LDS and row-linear kernels serve it)
    strided("strided-ks3-s2-origin0", 2, 16, 32, 64, 64, 3, 2, 0)
    strided("strided-ks3-s2-origin1", 2, 16, 32, 64, 64, 3, 2, 1)
    strided("strided-ks3-s2-origin0-f32", 2, 16, 32, 64, 64, 3, 2, 0, F32)
    strided("strided-ks3-s2-origin1-cin3", 2, 16, 32, 3, 64, 3, 2, 1)
    strided("strided-ks3-s1-is-lds", 2, 16, 32, 64, 64, 3, 1, 0)
    strided("strided-ks3-s1-small-map", 2, 4, 4, 64, 64, 3, 1, 0)
    strided("strided-ks1-s1-p16", 1, 4, 4, 128, 64, 1, 1, 0)
    strided("strided-ks1-s1-lin_rows", 1, 1, 65536, 96, 96, 1, 1, 0)
    strided("strided-ks1-s2", 2, 16, 32, 64, 64, 1, 2, 0)
    strided("strided-ks1-s2-large", 1, 64, 2048, 64, 96, 1, 2, 0)
    assert len({r["id"] for r in rows}) == len(rows)
    return rows


def describe_args(row):
    """The arguments of s3d_conv_plan_describe for a row, in order (without the buffer)."""
    return (row["N"], row["H"], row["W"], row["cout"], row["cin0"], row["cin1"], row["ks"], row["prec"], row["fused_gn"],
            4 * ws_floats(row["ws"], row["N"], row["H"], row["W"], row["cout"]), row["nsplit_out"], row["Hin"], row["Win"],
            row["stride"], row["pad_origin"])


def run(codes_path):
    import ctypes as C
    import torch
    from slice3d_amd import _lib as L
    lib = L.load()
    sep = torch.zeros(4, 4, device="cuda")
    ms = torch.ones(4, device="cuda")
    codes = []
    for row in cases():
        n, h, w, cout, cin0, cin1, ks = (row[k] for k in ("N", "H", "W", "cout", "cin0", "cin1", "ks"))
        hin, win = (row["Hin"], row["Win"]) if row["Hin"] else (h, w)
        packed = torch.zeros(lib.s3d_conv_packed_bytes(cout, cin0, cin1, ks), dtype=torch.uint8, device="cuda")
        x0 = torch.zeros(n, hin, win, pad16(cin0), device="cuda")
        x1 = torch.zeros(n, hin, win, pad16(cin1), device="cuda") if cin1 else None
        out = torch.zeros(n, h, w, cout, device="cuda")
        nws = ws_floats(row["ws"], n, h, w, cout)
        ws = torch.zeros(nws, device="cuda") if nws else None
        wsp, wsb = (ws.data_ptr(), 4 * nws) if nws else (None, 0)
        table = torch.zeros(n, 2, cin0 + cin1, device="cuda") if row["fused_gn"] else None
        torch.cuda.synchronize()
        L.check(lib.s3d_image_normalize_fwd(sep.data_ptr(), ms.data_ptr(), ms.data_ptr(), sep.data_ptr(), 1, 4, 2, 2, None),
                "separator")
        x1p = x1.data_ptr() if cin1 else None
        if row["Hin"]:
            rc = lib.s3d_conv_strided_fwd(packed.data_ptr(), x0.data_ptr(), out.data_ptr(), n, hin, win, h, w, cout, cin0, ks,
                                          row["stride"], row["pad_origin"], row["prec"], None)
        elif row["fused_gn"]:
            ns = C.c_int(0)
            rc = lib.s3d_conv_gn_fwd(packed.data_ptr(), x0.data_ptr(), x1p, None, out.data_ptr(), n, h, w, cout, cin0, cin1, ks,
                                     row["prec"], table.data_ptr(), 1, wsp, wsb, C.byref(ns) if row["nsplit_out"] else None, None)
        else:
            rc = lib.s3d_conv_fwd(packed.data_ptr(), x0.data_ptr(), x1p, None, out.data_ptr(), n, h, w, cout, cin0, cin1, ks,
                                  row["prec"], wsp, wsb, None)
        torch.cuda.synchronize()
        codes.append([row["id"], int(rc)])
        print("%-48s rc=%d" % (row["id"], rc), flush=True)
    with open(codes_path, "w") as f:
        json.dump(codes, f)


def kernel_name(raw):
    """`void f<1, true>(ConvLaunch, int) [clone .kd]` -> `f<1,true>`."""
    s = re.sub(r"\s*\[clone[^\]]*\]|\.kd$", "", raw.strip())
    s = re.sub(r"^void\s+", "", s)
    depth = 0
    for i, ch in enumerate(s):   # cut the argument list: the first '(' outside the template brackets
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            s = s[:i]
            break
    return s.replace(" ", "")


def from_trace(path, codes_path, commit, out):
    with open(path, newline="") as f:
        recs = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    groups = None
    for r in recs:
        name = kernel_name(r["Kernel_Name"])
        if name == SEPARATOR:
            groups = (groups or []) + [[]]
        elif groups is not None and re.match(r"(conv|lin_rows|lin_stream)", name):   # the engine's kernels, not torch's fills
            bx, by = int(r["Workgroup_Size_X"]), int(r["Workgroup_Size_Y"])
            groups[-1].append([name, int(r["Grid_Size_X"]) // bx, int(r["Grid_Size_Y"]) // by, bx])
    rows = cases()
    codes = json.load(open(codes_path))
    assert len(groups) == len(rows) == len(codes), (len(groups), len(rows), len(codes))
    for row, g, (rid, rc) in zip(rows, groups, codes):
        assert rid == row["id"]
        row["refused"] = int(rc != 0)
        row["kernels"] = g
        assert bool(g) != bool(rc), (rid, rc, g)
    doc = {"produced_by": "tools/conv_plan_sweep.py --run under rocprofv3 --kernel-trace on one MI355X, library of commit %s "
                          "(the dispatcher before the planner existed)" % commit,
           "kernel_fields": ["name", "grid_x", "grid_y", "block"], "rows": rows}
    with open(out, "w") as f:
        f.write('{"produced_by": %s, "kernel_fields": %s, "rows": [\n' % (json.dumps(doc["produced_by"]),
                                                                          json.dumps(doc["kernel_fields"])))
        f.write(",\n".join(json.dumps(r) for r in rows))
        f.write("\n]}\n")
    print("%d rows, %d kernel launches -> %s" % (len(rows), sum(len(g) for g in groups), out))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--from-trace", metavar="kernel_trace.csv")
    ap.add_argument("--codes", default="conv_plan_sweep_codes.json", help="return code per row: written by --run, read by --from-trace")
    ap.add_argument("--commit", default="?")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "conv_plan_sweep.json"))
    a = ap.parse_args()
    if a.list:
        for r in cases():
            print(r)
    elif a.run:
        run(a.codes)
    elif a.from_trace:
        from_trace(a.from_trace, a.codes, a.commit, a.out)


if __name__ == "__main__":
    main()
