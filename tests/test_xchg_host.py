"""The native exchange library without a GPU (include/clrrt_xchg.h, libclrrt_xchg.so): the header as C and as C++, the
exported entry points, the ctypes layout of clrrt_exchange_io against the C compiler's, argument checking (every bad
argument is refused with CLRRT_EINVAL before any device call), and the in-process transport's host rendezvous
(cl-rrt_amd/csrc/clrrt_rendezvous.hpp, no HIP) in a stand-alone program under ThreadSanitizer."""
import ctypes as C
import os
import subprocess

import pytest

from clrrt import abi
from clrrt import dist as cdist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
LIBX = os.path.join(ROOT, "cl-rrt_amd", "libclrrt_xchg.so")
EINVAL = -1

ENTRY_POINTS = ["clrrt_xchg_last_error", "clrrt_xchg_unique_id", "clrrt_xchg_create_rccl", "clrrt_xchg_group_create",
                "clrrt_xchg_group_destroy", "clrrt_xchg_create_local", "clrrt_xchg_hook", "clrrt_xchg_attach",
                "clrrt_xchg_records", "clrrt_xchg_stats", "clrrt_xchg_destroy", "clrrt_xchg_selftest_concat"]


@pytest.mark.parametrize("lang,std", [("c", "c99"), ("c++", "c++17")])
def test_header_compiles_as_c_and_cpp(lang, std):
    subprocess.run(["gcc", "-x", lang, f"-std={std}", "-Wall", "-Werror", "-fsyntax-only", "-I", INC,
                    os.path.join(INC, "clrrt_xchg.h")], check=True)


def test_library_exports_the_entry_points():
    assert os.path.exists(LIBX), "libclrrt_xchg.so not built (make -C cl-rrt_amd/csrc)"
    out = subprocess.run(["nm", "-D", "--defined-only", LIBX], capture_output=True, text=True, check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(ENTRY_POINTS) <= have, set(ENTRY_POINTS) - have


def test_engine_library_has_no_rccl_dependency():
    out = subprocess.run(["readelf", "-d", os.path.join(ROOT, "cl-rrt_amd", "libclrrt.so")], capture_output=True,
                         text=True, check=True).stdout
    assert "rccl" not in out and "clrrt_xchg" not in out


def test_exchange_io_ctypes_layout_is_the_c_layout(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "clrrt_xchg.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(clrrt_exchange_io), '
                   'offsetof(clrrt_exchange_io, stream), offsetof(clrrt_exchange_io, dev_all), '
                   'offsetof(clrrt_exchange_io, aux_sum), sizeof(clrrt_node)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", INC, "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    io = abi.ExchangeIO
    assert got == [C.sizeof(io), io.stream.offset, io.dev_all.offset, io.aux_sum.offset, C.sizeof(abi.Node)]
    assert cdist.REC_BYTES == got[4]


def test_bad_arguments_are_einval():
    L = cdist.xchg_lib()
    uid = (C.c_ubyte * cdist.UID_BYTES)()
    h = C.c_void_p()
    g = C.c_void_p()
    assert L.clrrt_xchg_unique_id(None) == EINVAL
    assert b"null" in L.clrrt_xchg_last_error()
    # (uid, rank, world, device, cap_records, first_bound, out)
    for args in [(None, 0, 1, 0, 16, 8), (uid, 2, 2, 0, 16, 8), (uid, -1, 2, 0, 16, 8), (uid, 0, 0, 0, 16, 8),
                 (uid, 0, 65, 0, 16, 8), (uid, 0, 1, -1, 16, 8), (uid, 0, 1, 0, 0, 8), (uid, 0, 1, 0, 16, 0)]:
        assert L.clrrt_xchg_create_rccl(*args, C.byref(h)) == EINVAL, args
        assert not h.value
    assert L.clrrt_xchg_create_rccl(uid, 0, 1, 0, 16, 8, None) == EINVAL
    for world, tmo in [(0, 100), (65, 100), (2, 0), (2, -5)]:
        assert L.clrrt_xchg_group_create(world, tmo, C.byref(g)) == EINVAL, (world, tmo)
    assert L.clrrt_xchg_group_create(2, 100, None) == EINVAL
    assert L.clrrt_xchg_group_create(2, 100, C.byref(g)) == 0 and g.value
    try:
        assert L.clrrt_xchg_create_local(None, 0, 0, 16, 8, C.byref(h)) == EINVAL
        for rank, dev, cap, fb in [(2, 0, 16, 8), (-1, 0, 16, 8), (0, -1, 16, 8), (0, 0, 0, 8), (0, 0, 16, 0)]:
            assert L.clrrt_xchg_create_local(g, rank, dev, cap, fb, C.byref(h)) == EINVAL, (rank, dev, cap, fb)
            assert not h.value
        assert L.clrrt_xchg_create_local(g, 0, 0, 16, 8, None) == EINVAL
    finally:
        L.clrrt_xchg_group_destroy(g)
    io = abi.ExchangeIO()
    assert L.clrrt_xchg_hook(None, C.byref(io)) == -1
    assert L.clrrt_xchg_attach(None, None) == EINVAL
    assert L.clrrt_xchg_stats(None, (C.c_int64 * 8)()) == EINVAL
    assert L.clrrt_xchg_records(None) is None
    L.clrrt_xchg_destroy(None)  # a no-op
    # the kernel's selftest checks its arguments before it touches a device
    el, aux, bb = (C.c_double * 2)(), (C.c_int64 * 2)(), (C.c_double * 8)()
    out, summ = (C.c_ubyte * (160 * 16))(), (C.c_int64 * 10)()

    def concat(W, bound, counts, excess=0, out_cap=16):
        return L.clrrt_xchg_selftest_concat(0, W, bound, (C.c_int32 * 2)(*counts), el, aux, bb, excess, out, out_cap, summ)

    assert concat(0, 4, (1, 1)) == EINVAL
    assert concat(65, 4, (1, 1)) == EINVAL
    assert concat(2, 0, (0, 0)) == EINVAL
    assert concat(2, 4, (-1, 1)) == EINVAL
    assert concat(2, 4, (5, 1)) == EINVAL          # above bound without excess rows
    assert concat(2, 4, (8, 1), excess=3) == EINVAL  # above bound + excess rows
    assert concat(2, 4, (4, 4), out_cap=7) == EINVAL


def test_rendezvous_under_thread_sanitizer(tmp_path):
    """2, 3 and 8 threads over 1000 rounds of publish / meet / read the peers / meet, then a peer that never arrives:
    a stand-alone host program (its own main, nothing loaded into Python), built with -fsanitize=thread."""
    exe = tmp_path / "rendezvous_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "rendezvous_check.cpp"), "-lpthread"], check=True)
    r = subprocess.run([str(exe), "1000"], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-3000:])
    assert r.returncode == 0 and "failures 0" in r.stdout
    assert "ThreadSanitizer" not in r.stderr
    assert r.stdout.count(": ok") == 4
