"""The fixed-order workgroup sum of csrc/hl_reduce.h, pinned to its stated order rather than to run-to-run equality:
hl_adamw_sum_partials (strided_sum + block_sum in one workgroup) against a numpy restatement of that order, byte for byte."""
import ctypes as C

import numpy as np
import pytest
import torch

from humanliff_amd import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
THREADS = 256          # kReduceThreads


def restated(p):
    """acc[t] = p[t] + p[t + 256] + ... left to right; then for s = 128, 64, ..., 1: acc[t] += acc[t + s] for t < s."""
    acc = np.zeros(THREADS, np.float64)
    for t in range(min(THREADS, p.size)):
        for v in p[t::THREADS]:
            acc[t] = acc[t] + v
    s = THREADS // 2
    while s:
        acc[:s] += acc[s:2 * s]
        s //= 2
    return acc[0]


def sequential(p):
    tot = np.float64(0.0)
    for v in p:
        tot = tot + v
    return tot


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])      # one element, one short of a pass, one pass, the first wrap, several wraps
def test_sum_partials_follows_the_stated_order(n):
    rng = np.random.default_rng(100 + n)
    p = rng.choice([-1, 1], n) * 10 ** rng.uniform(-8, 8, n)
    want = restated(p)
    if n >= 255:         # the order must matter for these inputs, or the comparison below would pin nothing
        assert want.tobytes() != sequential(p).tobytes()
        assert want.tobytes() != np.float64(np.sum(p)).tobytes()
    d = torch.from_numpy(p).to(DEV)
    out = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
    _lib.check(_lib.lib().hl_adamw_sum_partials(C.c_void_p(d.data_ptr()), n, C.c_void_p(out.data_ptr()), _lib.stream_ptr()),
               "hl_adamw_sum_partials")
    got = out.cpu().numpy()
    assert got.tobytes() == np.float64(want).tobytes()
