"""The UNet forward's GroupNorm-statistics registry (csrc/hl_stat_book.h) without a GPU: the header is compiled as plain C++ into a small shared
library and called through ctypes.  The registry decides whether a consumer may read the group totals its producers left; a wrong answer would
show in the network only as a last-bits or run-to-run difference, so every rule is pinned here alone.  Pointers are fake: integers, never
dereferenced (channel c of a buffer at address a lies at a + 4 c)."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "humanliff_amd", "csrc")

_SRC = r"""
#include <cstdint>
#include "hl_stat_book.h"
static const float *P(intptr_t a) { return reinterpret_cast<const float *>(a); }
static float *B(intptr_t a) { return reinterpret_cast<float *>(a); }
extern "C" {
void *book_new() { return new hl::StatBook(); }
void book_free(void *b) { delete static_cast<hl::StatBook *>(b); }
void book_concat_halves(void *b, intptr_t cat, int C, int split, intptr_t buf) { static_cast<hl::StatBook *>(b)->concat_halves(P(cat), C, split, B(buf)); }
void book_block_for(void *b, intptr_t out, int Cout, intptr_t fallback, intptr_t *buf, int *viewC, int *c0) {
    const hl::StatBook::Block k = static_cast<const hl::StatBook *>(b)->block_for(P(out), Cout, B(fallback));
    *buf = reinterpret_cast<intptr_t>(k.buf); *viewC = k.viewC; *c0 = k.c0;
}
int book_in_concat(void *b, intptr_t out) { return static_cast<const hl::StatBook *>(b)->in_concat(P(out)) ? 1 : 0; }
void book_produced(void *b, intptr_t p, intptr_t buf, int viewC, int c0, int covered) {
    static_cast<hl::StatBook *>(b)->produced(P(p), hl::StatBook::Block{B(buf), viewC, c0}, covered);
}
void book_stored_without_totals(void *b, intptr_t p) { static_cast<hl::StatBook *>(b)->stored_without_totals(P(p)); }
intptr_t book_totals_of(void *b, intptr_t p, int C, int need_view_match) {
    return reinterpret_cast<intptr_t>(static_cast<const hl::StatBook *>(b)->totals_of(P(p), C, need_view_match != 0));
}
}
"""

_I, _P = ctypes.c_int, ctypes.c_ssize_t       # (intptr_t)


@pytest.fixture(scope="module")
def booklib(tmp_path_factory):
    from humanliff_amd import build
    tmp = tmp_path_factory.mktemp("stat_book")
    src, lib = str(tmp / "book.cpp"), str(tmp / "libbook.so")
    with open(src, "w") as f:
        f.write(_SRC)
    r = subprocess.run([build.HIPCC, "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-I", CSRC, src, "-o", lib], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    L = ctypes.CDLL(lib)
    for name, res, args in [("book_new", ctypes.c_void_p, []), ("book_free", None, [ctypes.c_void_p]),
                            ("book_concat_halves", None, [ctypes.c_void_p, _P, _I, _I, _P]),
                            ("book_block_for", None, [ctypes.c_void_p, _P, _I, _P, ctypes.POINTER(_P), ctypes.POINTER(_I), ctypes.POINTER(_I)]),
                            ("book_in_concat", _I, [ctypes.c_void_p, _P]),
                            ("book_produced", None, [ctypes.c_void_p, _P, _P, _I, _I, _I]),
                            ("book_stored_without_totals", None, [ctypes.c_void_p, _P]),
                            ("book_totals_of", _P, [ctypes.c_void_p, _P, _I, _I])]:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


class Book:
    """One hl::StatBook; addresses are plain integers, 0 is the null pointer."""

    def __init__(self, L):
        self.L, self.h = L, L.book_new()

    def __del__(self):
        self.L.book_free(self.h)

    def concat_halves(self, cat, C, split, buf):
        self.L.book_concat_halves(self.h, cat, C, split, buf)

    def block_for(self, out, Cout, fallback):
        buf, viewC, c0 = _P(-1), _I(-1), _I(-1)
        self.L.book_block_for(self.h, out, Cout, fallback, ctypes.byref(buf), ctypes.byref(viewC), ctypes.byref(c0))
        return buf.value, viewC.value, c0.value

    def in_concat(self, out):
        return bool(self.L.book_in_concat(self.h, out))

    def produced(self, p, block, covered):
        self.L.book_produced(self.h, p, block[0], block[1], block[2], covered)

    def stored_without_totals(self, p):
        self.L.book_stored_without_totals(self.h, p)

    def totals_of(self, p, C, need_view_match=False):
        return self.L.book_totals_of(self.h, p, C, int(need_view_match))


X, CAT = 0x10000, 0x40000            # tensors
S1, S2, S3 = 0x900000, 0x901000, 0x902000   # statistics blocks
C, CH = 96, 64                        # a concat of 96 channels split at 64: halves at CAT and CAT + 4 * 64
HALF2 = CAT + 4 * CH


def _concat(L, second_block=None, produce_second=True):
    """Both halves of a declared concat produced the way Exec::conv does it: the block comes from block_for."""
    b = Book(L)
    b.concat_halves(CAT, C, CH, S1)
    b.produced(CAT, b.block_for(CAT, CH, S2), CH)
    if produce_second:
        blk = b.block_for(HALF2, C - CH, S3)
        b.produced(HALF2, blk if second_block is None else (second_block, blk[1], blk[2]), C - CH)
    return b


def test_single_producer(booklib):
    b = Book(booklib)
    assert b.totals_of(X, C) == 0 and b.totals_of(X, C, True) == 0          # nothing recorded
    b.produced(X, (S1, C, 0), C)
    assert b.totals_of(X, C) == S1 and b.totals_of(X, C, True) == S1
    # totals grouped for another view: good for the sum x^2 of the tensor, not for its GroupNorm
    b.produced(X, (S1, 2 * C, 0), C)
    assert b.totals_of(X, C) == S1 and b.totals_of(X, C, True) == 0


def test_concat_both_halves(booklib):
    b = _concat(booklib)
    assert b.totals_of(CAT, C) == S1 and b.totals_of(CAT, C, True) == S1


def test_concat_one_half_produced(booklib):
    b = _concat(booklib, produce_second=False)
    assert b.totals_of(CAT, C) == 0 and b.totals_of(CAT, C, True) == 0


def test_concat_without_a_shared_block(booklib):
    b = _concat(booklib, second_block=S3)
    assert b.totals_of(CAT, C) == 0 and b.totals_of(CAT, C, True) == 0


def test_concat_second_half_stored_without_totals(booklib):
    """The skip-convolution and memcpy paths: a later store without totals withdraws what the producer recorded."""
    b = _concat(booklib)
    assert b.totals_of(CAT, C) == S1
    b.stored_without_totals(HALF2)
    assert b.totals_of(CAT, C) == 0 and b.totals_of(CAT, C, True) == 0
    b.stored_without_totals(HALF2)                                           # (nothing to withdraw: no effect)
    assert b.totals_of(CAT, C) == 0


def test_superset_is_refused(booklib):
    """A block that covers more channels than the tensor asked for may still be growing: never handed out."""
    b = Book(booklib)
    b.produced(X, (S1, C, 0), C)
    assert b.totals_of(X, CH) == 0 and b.totals_of(X, CH, True) == 0
    assert b.totals_of(X, C + 32) == 0                                       # nor does a record that covers less than the tensor
    c = _concat(booklib)
    assert c.totals_of(CAT, C + 32) == 0 and c.totals_of(CAT, C - 16) == 0   # the two halves together must give exactly C


def test_part_only_is_refused(booklib):
    b = _concat(booklib)
    assert b.totals_of(HALF2, C - CH) == 0 and b.totals_of(HALF2, C - CH, True) == 0
    assert b.totals_of(CAT, CH, True) == 0                                   # the first half as a view of its own: grouped for the concat


def test_reproduction_later_record_wins(booklib):
    b = Book(booklib)
    b.produced(X, (S1, C, 0), C)
    b.produced(X, (S2, C, 0), C)
    assert b.totals_of(X, C, True) == S2
    b.stored_without_totals(X)
    assert b.totals_of(X, C) == 0
    b.produced(X, (S3, C, 0), C)
    assert b.totals_of(X, C, True) == S3


def test_block_lookup(booklib):
    b = Book(booklib)
    b.concat_halves(CAT, C, CH, S1)
    assert b.in_concat(CAT) and b.in_concat(HALF2) and not b.in_concat(X) and not b.in_concat(CAT + 4)
    assert b.block_for(CAT, CH, S2) == (S1, C, 0)                            # inside: the shared block, the concat's channel count, the half's first channel
    assert b.block_for(HALF2, C - CH, S2) == (S1, C, CH)
    assert b.block_for(X, 48, S2) == (S2, 48, 0)                             # outside: the fallback as a view of its own
    assert b.block_for(CAT + 4, 48, S3) == (S3, 48, 0)                       # (only the two declared addresses are halves)
    assert b.block_for(X, 48, 0) == (0, 48, 0)
