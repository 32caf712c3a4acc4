"""k_conv_h2s without a GPU: its register / scratch / LDS budget from the compiled metadata, and its 16x16x32 operand maps (h2s_px, h2s_kgrp,
h2s_wfrag_off in hl_conv_h16.hip) against the index formula of k_pack_conv_h2 and the ds_read_b128 bank rule."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "humanliff_amd", "csrc", "hl_conv_h16.hip")


def _kernel_metadata(name):
    from humanliff_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "h16.s")
        cmd = [build.HIPCC] + build.FLAGS + build.FILE_FLAGS.get("hl_conv_h16.hip", []) + ["--cuda-device-only", "-S", SRC, "-o", out]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode()
        text = open(out).read()
    meta = text[text.index(".amdgpu_metadata"):]
    for entry in re.split(r"\n  - ", meta):
        if re.search(r"\.name:\s+\S*" + name + r"ENS_5ConvKE\s*\n", entry):
            return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*\n", entry)}
    raise AssertionError(f"{name} not in the metadata")


def test_conv_h2s_register_and_lds_budget():
    """__launch_bounds__(256, 2): two workgroups per CU need <= 256 registers per lane (vector + accumulator), no scratch, no static LDS."""
    md = _kernel_metadata("k_conv_h2s")
    assert md["vgpr_count"] + md["agpr_count"] <= 256, md
    assert md["private_segment_fixed_size"] == 0, md
    assert md["vgpr_spill_count"] == 0, md
    assert md["group_segment_fixed_size"] == 0, md


# ---- the device helpers, line for line
def h2s_px(r):
    return r ^ (0 if r & 8 else 4)


def h2s_kgrp(kg):
    return ((kg & 1) << 1) | (kg >> 1)


def h2s_wfrag_off(wave, f, lane):
    o, g = 48 * wave + 16 * f + (lane & 15), h2s_kgrp(lane >> 4)
    k2, wn, nf, l = g >> 1, o // 96, (o % 96) // 32, (o & 31) + 32 * (g & 1)
    return k2 * 12288 + wn * 3072 + nf * 1024 + l * 16


def _packed_image_map(nb_count, nch):
    """k_pack_conv_h2's element i -> (output channel o, input channel cin, tap, plane), as the kernel decodes it."""
    n = nb_count * nch * 18 * 2 * 3072
    i = np.arange(n, dtype=np.int64)
    j, l = i & 7, (i >> 3) & 63
    t = i >> 9
    nf = t % 3; t //= 3
    wn = t & 1; t >>= 1
    pl = t & 1; t >>= 1
    k2 = t & 1; t >>= 1
    tap = t % 9; t //= 9
    chunk = t % nch
    nb = t // nch
    o = nb * 192 + wn * 96 + nf * 32 + (l & 31)
    cin = chunk * 32 + k2 * 16 + (l >> 5) * 8 + j
    return o, cin, tap, pl


def test_conv_h2s_b_fragments_match_the_packed_image():
    """Lane L of B fragment f of wave w, k-step (chunk, tap), plane pl: 8 consecutive fp16 values at byte
    wbase + (chunk * 9 + tap) * 24576 + pl * 6144 + h2s_wfrag_off(w, f, L) must be output channel 48 w + 16 f + (L & 15) of the block and inputs
    32 chunk + 8 h2s_kgrp(L >> 4) + 0..7 - the same k-group the A fragment of that lane reads."""
    nb_count, nch = 2, 3
    o, cin, tap, pl = _packed_image_map(nb_count, nch)
    for nb in range(nb_count):
        wbase = nb * nch * 18 * 6144 * 2
        for chunk in range(nch):
            for tp in range(9):
                for plane in range(2):
                    for wave in range(4):
                        for f in range(3):
                            for lane in range(64):
                                off = wbase + (chunk * 9 + tp) * 24576 + plane * 6144 + h2s_wfrag_off(wave, f, lane)
                                assert off % 16 == 0
                                e = off // 2 + np.arange(8)
                                assert (o[e] == nb * 192 + 48 * wave + 16 * f + (lane & 15)).all()
                                assert (cin[e] == chunk * 32 + 8 * h2s_kgrp(lane >> 4) + np.arange(8)).all()
                                assert (tap[e] == tp).all() and (pl[e] == plane).all()


def test_conv_h2s_fragment_maps_are_permutations():
    assert sorted(h2s_px(r) for r in range(16)) == list(range(16))
    assert sorted(h2s_kgrp(k) for k in range(4)) == list(range(4))
    # every (pixel slot, channel) of a wave's 128 x 48 block is written exactly once by the scatter of the 16x16 C layout
    for wave in range(4):
        seen = set()
        for mf in range(8):
            for f in range(3):
                for lane in range(64):
                    for i in range(4):
                        seen.add((16 * mf + h2s_px(4 * (lane >> 4) + i), 48 * wave + 16 * f + (lane & 15)))
        assert len(seen) == 128 * 48


# lane groups of one ds_read_b128 (each is served in its own LDS cycle set; its 16 lanes must hit 16 distinct 16-byte slots of a 256-byte bank row)
_B128_GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
_B128_GROUPS += [[l + 32 for l in g] for g in _B128_GROUPS]


def _a_addr(lane, kx, px_map, kg_map):
    px, g = px_map(lane & 15) + kx, kg_map(lane >> 4)
    return px * 64 + ((g ^ ((px >> 2) & 3)) << 4)


@pytest.mark.parametrize("kx", [0, 1, 2])
def test_conv_h2s_a_reads_are_conflict_free(kx):
    for grp in _B128_GROUPS:
        slots = [(_a_addr(l, kx, h2s_px, h2s_kgrp) // 16) % 16 for l in grp]
        assert len(set(slots)) == 16, (kx, grp, slots)
    # (the identity maps would not be: two lanes per slot in every group)
    grp = _B128_GROUPS[0]
    assert len({(_a_addr(l, kx, lambda r: r, lambda k: k) // 16) % 16 for l in grp}) < 16
