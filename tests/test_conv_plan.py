"""The convolution engine's planner (conv_plan.h) against the dispatcher it replaced, on a machine without a GPU.

tests/golden/conv_plan_sweep.json holds, per row of tools/conv_plan_sweep.py's case table, the kernels the library of the
commit named in its header launched (a rocprofv3 kernel trace on an MI355X): name, grid in workgroups, block, in order, the
split-K finish pass included.  s3d_conv_plan_describe must name exactly those for every row, and refuse the rows that
library refused.  Two coverage properties keep the conformance rows of tests/test_gpu_conv.py honest: every instantiation
profiles/conv_conformance_kernels.md lists as reached is in the golden, and every row id of that file that names an
instantiation is planned onto it."""
import ctypes as C
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import conv_plan_sweep as sweep  # noqa: E402

ENGINE = re.compile(r"(conv|lin_rows|lin_stream)")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "conv_plan_sweep.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib():
    from slice3d_amd import _lib as L
    assert not os.environ.get("S3D_CONV_SMALL") and not os.environ.get("S3D_CONV_SMALL_1X1"), "the golden is of the default tuning"
    return L.load()


def describe(lib, row):
    """(return code, [[kernel name, grid x, grid y, block], ...], text) of s3d_conv_plan_describe for a sweep row."""
    buf = C.create_string_buffer(512)
    rc = lib.s3d_conv_plan_describe(*sweep.describe_args(row), buf, len(buf))
    text = buf.value.decode() if rc == 0 else (lib.s3d_last_error() or b"").decode()
    kernels = []
    if rc == 0:
        for part in text.split("; "):
            m = re.match(r"(\S+) grid=(\d+)x(\d+) block=(\d+)", part)
            assert m, text
            kernels.append([m.group(1)] + [int(g) for g in m.groups()[1:]])
    return rc, kernels, text


def test_the_case_table_is_the_goldens(golden):
    rows = sweep.cases()
    assert len(golden["rows"]) == len(rows) and len(rows) >= 300
    for g, r in zip(golden["rows"], rows):
        assert {k: g[k] for k in r} == r, r["id"]


def test_planner_names_the_kernels_the_old_dispatcher_launched(golden, lib):
    bad = []
    for row in golden["rows"]:
        rc, kernels, text = describe(lib, row)
        if row["refused"]:
            if rc >= 0:
                bad.append((row["id"], "refused by the old dispatcher", text))
        elif rc != 0 or kernels != row["kernels"]:
            bad.append((row["id"], row["kernels"], text))
    assert not bad, "%d of %d rows differ, the first: %r" % (len(bad), len(golden["rows"]), bad[:5])


def test_plan_reports_split_count_and_deferred_finish(golden, lib):
    """splits = the grid's y of a split-K kernel; finish = 1 exactly when conv_splitk_finish_kernel follows."""
    for row in golden["rows"]:
        if row["refused"]:
            continue
        _, kernels, text = describe(lib, row)
        splits, finish = (int(v) for v in re.search(r"splits=(\d+) finish=(\d)", text).groups())
        assert finish == (kernels[-1][0] == "conv_splitk_finish_kernel"), (row["id"], text)
        assert finish == (splits > 1 and not row["nsplit_out"]), (row["id"], text)
        if re.match(r"conv3x3_(lds|small)", kernels[0][0]):
            assert splits == kernels[0][2], (row["id"], text)
        else:
            assert splits == 1, (row["id"], text)


def test_every_reached_instantiation_of_the_conformance_note_is_in_the_golden(golden):
    seen = {k[0] for row in golden["rows"] for k in row["kernels"]}
    listed = []
    with open(os.path.join(ROOT, "profiles", "conv_conformance_kernels.md")) as f:
        for line in f:
            m = re.match(r"\| `([^`*]+)` \| (\d+) \|", line)
            if m and ENGINE.match(m.group(1)):
                listed.append(m.group(1))
    assert len(listed) >= 50, listed
    # (the note cuts trailing default template arguments: `<4,2,2,2,false>` stands for `<4,2,2,2,false,false>`)
    missing = [n for n in listed if not any(s == n or (n.endswith(">") and s.startswith(n[:-1] + ",")) for s in seen)]
    assert not missing, missing


def _named_instantiation(rid):
    """Regular expression of the kernel a tests/test_gpu_conv.py row id names (at PREC_F16X3), or None."""
    gn = "true" if "_gn" in rid else "false"
    m = re.match(r"lds_(\d)_(\d)_(\d)_(\d|x)", rid)
    if m:
        return r"conv3x3_lds_f16x3_kernel<%s,%s,%s,%s,%s,false>" % (m.group(1), m.group(2), m.group(3), m.group(4).replace("x", r"\d"), gn)
    m = re.match(r"small(3x3|1x1)_pt(\d)", rid)
    if m:
        return r"conv3x3_small_f16x3_kernel<%s,%s,%s>" % (m.group(2), gn, 9 if m.group(1) == "3x3" else 1)
    m = re.match(r"lin_stream_(\d)", rid)
    if m:
        return r"lin_stream_f16x3_kernel<%s>" % m.group(1)
    if rid.startswith("lin_rows"):
        return r"lin_rows_f16x3_kernel"
    m = re.match(r"(?:menu|strided_f16x3)_(\d)_(\d)_(\d)_(\d)-ks(\d)", rid)
    if m:
        return r"conv_igemm_f16x3_kernel<%s,%s,%s,%s,%s,false>" % m.groups()
    if rid.startswith("strided_f16x3"):
        return r"conv_igemm_f16x3_kernel<.*>"
    if "fp32" in rid:
        return r"conv_igemm_kernel<.*>"
    return None


def test_conformance_row_ids_name_the_kernel_they_are_planned_onto(golden, lib):
    """The id of a tests/test_gpu_conv.py row names its instantiation in the split-precision mode, with a large workspace
    where the row takes one."""
    by_id = {row["id"]: row for row in golden["rows"]}
    fwd, gn, strided = sweep._test_tables()
    checked = 0
    for name, ws in [(c[0], "big" if c[10] else "none") for c in fwd] + [(c[0], "big") for c in gn] + [(c[0], None) for c in strided]:
        pattern = _named_instantiation(name)
        assert pattern, name
        row = by_id["t:%s/f16x3" % name if ws is None else "t:%s/%s/f16x3" % (name, ws)]
        rc, kernels, text = describe(lib, row)
        assert rc == 0 and re.fullmatch(pattern, kernels[0][0]), (name, pattern, text)
        if "splitk" in name:
            assert kernels[0][2] > 1, (name, text)
        checked += 1
    assert checked == len(fwd) + len(gn) + len(strided) >= 45


def test_refusals_keep_their_messages(lib):
    buf = C.create_string_buffer(256)
    # a fused GroupNorm off the LDS-staged kernel's shapes, ks 2, a strided call with a workspace
    assert lib.s3d_conv_plan_describe(2, 16, 32, 48, 64, 0, 3, 1, 1, 0, 0, 0, 0, 0, 0, buf, len(buf)) == -1
    assert b"s3d_conv_gn_supported" in lib.s3d_last_error()
    assert lib.s3d_conv_plan_describe(2, 16, 32, 64, 64, 0, 2, 1, 0, 0, 0, 0, 0, 0, 0, buf, len(buf)) == -1
    assert b"conv_fwd: bad arguments" in lib.s3d_last_error()
    assert lib.s3d_conv_plan_describe(2, 8, 16, 64, 64, 0, 3, 1, 0, 4096, 0, 16, 32, 2, 0, buf, len(buf)) == -1
    assert lib.s3d_conv_plan_describe(2, 8, 16, 64, 64, 0, 3, 1, 0, 0, 0, 16, 32, 2, 0, None, 0) == -1
