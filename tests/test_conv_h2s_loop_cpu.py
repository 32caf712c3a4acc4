"""The chunk loops of the fp16x2 stride-1 kernels (every entry point whose name starts with k_conv_h2s or k_conv1_h2s) without a GPU, from the
ISA hl_conv_h16.hip compiles to (the build line of tests/test_conv_h2s_tiles_cpu.py):
  1. no buffer operation sits in a waterfall loop (the activation descriptor is built from provably wave-uniform values);
  2. the innermost loop that holds the MFMAs - one chunk - is ONE basic block: its only scalar-condition branches are its own back edge and
     its exit (the staging mode is a template parameter, not a run-time branch inside the chunk);
  3. in the affine instantiations no coefficient read is waited on where it is issued: between the last MFMA in front of a full
     s_waitcnt lgkmcnt(0) and that wait there is no ds_read_b128 (the quads are read a fragment row ahead of the staging that uses them);
  4. every entry point keeps two workgroups per CU: <= 256 registers, no scratch, no spills, no static LDS.
The test searches for these patterns only."""
import functools
import os
import re
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "humanliff_amd", "csrc", "hl_conv_h16.hip")
PREFIXES = ("k_conv_h2s", "k_conv1_h2s")
# the instantiations that apply the GroupNorm coefficients while they stage
AFFINE = ("k_conv_h2s", "k_conv_h2s_aff", "k_conv1_h2s_aff", "k_conv1_h2s_aff_silu")
EXPECTED = {"k_conv_h2s", "k_conv_h2s_aff", "k_conv_h2s_raw", "k_conv_h2s_planes", "k_conv_h2s_ph", "k_conv1_h2s", "k_conv1_h2s_aff", "k_conv1_h2s_aff_silu"}


@functools.lru_cache(maxsize=None)
def _isa():
    from humanliff_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "h16.s")
        cmd = [build.HIPCC] + build.FLAGS + build.FILE_FLAGS.get("hl_conv_h16.hip", []) + ["--cuda-device-only", "-S", SRC, "-o", out]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode()
        return open(out).read()


def _short(mangled):
    """_ZN2hl12_GLOBAL__N_110k_conv_h2sENS_5ConvKE -> k_conv_h2s (None: not a kernel taking a ConvK in hl's anonymous namespace)."""
    m = re.match(r"_ZN2hl12_GLOBAL__N_1(\d+)", mangled)
    if not m or not mangled.endswith("ENS_5ConvKE"):
        return None
    name = mangled[m.end():m.end() + int(m.group(1))]
    return name if mangled == m.group(0) + name + "ENS_5ConvKE" else None


@functools.lru_cache(maxsize=None)
def _kernels():
    """{short name: (instruction lines of the body, metadata ints)} of the kernels under test."""
    text = _isa()
    bodies, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            bodies[cur] = []
        elif line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and line.strip() and not line.lstrip().startswith(";"):
            bodies[cur].append(line)
    meta = {}
    for entry in re.split(r"\n  - ", text[text.index(".amdgpu_metadata"):]):
        m = re.search(r"\.name:\s+(\S+)\s*\n", entry)
        if m:
            meta[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*\n", entry)}
    out = {}
    for mangled, body in bodies.items():
        name = _short(mangled)
        if name and name.startswith(PREFIXES) and mangled in meta:
            out[name] = (body, meta[mangled])
    return out


def _names():
    return sorted(EXPECTED)


def test_the_entry_points_are_the_expected_ones():
    assert set(_kernels()) == EXPECTED


def _op(line):
    s = line.strip()
    return "" if s.startswith(".") or s.endswith(":") else s.split()[0]


def _mfma_loop(body):
    """(first, last) line index of the innermost loop that holds MFMAs: the shortest backward branch whose span has one."""
    labels = {m.group(1): i for i, l in enumerate(body) if (m := re.match(r"^(\.LBB\w+):", l))}
    loops = []
    for i, l in enumerate(body):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\w+)", l)
        if m and labels.get(m.group(1), i) < i and any(_op(x).startswith("v_mfma") for x in body[labels[m.group(1)]:i]):
            loops.append((i - labels[m.group(1)], labels[m.group(1)], i))
    assert loops, "no loop with MFMAs"
    _, a, b = min(loops)
    return a, b, labels


@pytest.mark.parametrize("name", _names())
def test_no_waterfall_around_a_buffer_operation(name):
    body, _ = _kernels()[name]
    ops = [_op(l) for l in body]
    n_buf = 0
    for i, op in enumerate(ops):
        if op.startswith(("buffer_load", "buffer_store")):
            n_buf += 1
            assert "s_cbranch_execnz" not in ops[i + 1:i + 5], (name, i, body[i:i + 5])
    assert n_buf > 0


@pytest.mark.parametrize("name", _names())
def test_the_chunk_is_one_basic_block(name):
    body, _ = _kernels()[name]
    a, b, labels = _mfma_loop(body)
    n_mfma = sum(_op(l).startswith("v_mfma") for l in body[a:b + 1])
    assert n_mfma == sum(_op(l).startswith("v_mfma") for l in body), (name, "MFMAs outside the chunk loop")
    for i in range(a, b + 1):
        m = re.match(r"\s+(s_cbranch_(?:scc|vcc)\w*)\s+(\.LBB\w+)", body[i])
        if not m:
            continue
        t = labels[m.group(2)]
        back_edge = i == b and t == a
        leaves = t > b or t < a
        assert back_edge or leaves, (name, i - a, body[i].strip(), "a scalar-condition branch inside the chunk")
    # and nothing but the back edge jumps backwards inside it
    for i in range(a, b):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\w+)", body[i])
        assert not (m and a <= labels[m.group(1)] <= i), (name, i - a, body[i].strip())


@pytest.mark.parametrize("name", AFFINE)
def test_no_coefficient_read_is_waited_on_where_it_is_issued(name):
    body, _ = _kernels()[name]
    a, b, _ = _mfma_loop(body)
    ops = [(_op(l), l) for l in body[a:b + 1]]
    since_mfma, waits = 0, 0
    for op, line in ops:
        if op.startswith("v_mfma"):
            since_mfma = 0
        elif op == "ds_read_b128":
            since_mfma += 1
        elif op == "s_waitcnt" and re.search(r"lgkmcnt\(0\)", line):
            waits += 1
            assert since_mfma == 0, (name, line.strip(), f"{since_mfma} ds_read_b128 between the last MFMA and this wait")
    print(f"{name}: {waits} full LDS waits in the chunk")


@pytest.mark.parametrize("name", _names())
def test_register_and_lds_budget(name):
    _, md = _kernels()[name]
    assert md["vgpr_count"] + md["agpr_count"] <= 256, md
    assert md["private_segment_fixed_size"] == 0, md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
    assert md["group_segment_fixed_size"] == 0, md
