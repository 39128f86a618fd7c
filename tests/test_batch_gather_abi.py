"""CPU checks of dl_batch_gather's C ABI: the struct layout agrees between C and ctypes, the
symbol is additive (ABI still 10), every refusal the header states comes back with its status
and a message before any device call (dummy pointers, runs without a GPU), and the host-only
checker (csrc/launch.cpp shape_batch_gather) accepts the valid call shapes and shapes their
launches -- the latter from a small stand-alone program built with the address and
undefined-behaviour sanitizers and run as an ordinary process."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "distributed-learning_amd", "csrc")

FIELDS = ["samples", "ld_samples", "targets", "n_samples", "dim", "index", "s_index", "n_agents",
          "batch", "steps", "cursor", "step", "advance", "data", "s_data", "labels", "s_labels"]


def test_struct_layout_matches_c(tmp_path):
    from distributed_learning_amd import _lib
    offs = "".join(f'printf("%zu ", offsetof(dl_batch_gather_args, {f}));' for f in FIELDS)
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dlamd.h"\n'
                    'int main(void){printf("%zu ", sizeof(dl_batch_gather_args));' + offs +
                    'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)],
                   check=True)
    c = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                        check=True).stdout.split()]
    A = _lib.DlBatchGatherArgs
    assert [f for f, _ in A._fields_] == FIELDS
    assert c == [ctypes.sizeof(A)] + [getattr(A, f).offset for f in FIELDS]


def test_symbol_is_additive():
    from distributed_learning_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "dl_batch_gather")
    assert "dl_batch_gather" in _lib.SIGNATURES
    assert lib.dl_abi_version() == 10 == _lib.ABI_VERSION


# dummy device addresses, never dereferenced, far apart
SAMPLES, TARGETS, INDEX, CURSOR, DATA, LABELS = (1 << 32, 1 << 40, 1 << 41, 1 << 42, 1 << 43,
                                                 1 << 44)
M, DIM, N, B, S = 60000, 784, 8, 64, 5


def valid(**kw):
    from distributed_learning_amd import _lib
    a = _lib.DlBatchGatherArgs(SAMPLES, DIM, TARGETS, M, DIM, INDEX, S * B, N, B, S, CURSOR, 0, 1,
                               DATA, B * DIM, LABELS, B)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def refused(a):
    """(status, message) of a call that must be refused before any device call."""
    from distributed_learning_amd import _lib
    lib = _lib.load()
    rc = lib.dl_batch_gather(ctypes.byref(a) if a is not None else None, None)
    return rc, lib.dl_last_error()


def test_refusals():
    from distributed_learning_amd import _lib
    INV = _lib.DL_ERR_INVALID
    rc, msg = refused(None)
    assert rc == INV and b"args is NULL" in msg
    for f in ("n_agents", "batch", "steps", "n_samples"):
        for v in (0, -1):
            rc, msg = refused(valid(**{f: v}))
            assert rc == INV and b">= 1" in msg, (f, v, msg)
    for d in (0, -4, 2, 786, 783):
        rc, msg = refused(valid(dim=d, ld_samples=1024, s_data=B * 1024))
        assert rc == INV and b"dim must be" in msg, (d, msg)
    for f in ("samples", "index", "data"):
        rc, msg = refused(valid(**{f: None}))
        assert rc == INV and b"null samples, index or data" in msg, (f, msg)
    for ld in (DIM - 4, DIM + 2, 0):
        rc, msg = refused(valid(ld_samples=ld))
        assert rc == INV and b"ld_samples" in msg, (ld, msg)
    for sd in (B * DIM - 4, B * DIM + 2, 0):
        rc, msg = refused(valid(s_data=sd))
        assert rc == INV and b"s_data" in msg, (sd, msg)
    for si in (S * B - 1, 1, -S * B):
        rc, msg = refused(valid(s_index=si))
        assert rc == INV and b"s_index" in msg, (si, msg)
    rc, msg = refused(valid(samples=SAMPLES + 4))
    assert rc == INV and b"16-byte aligned" in msg
    rc, msg = refused(valid(data=DATA + 8))
    assert rc == INV and b"16-byte aligned" in msg
    rc, msg = refused(valid(targets=None))                       # labels without targets
    assert rc == INV and b"labels need targets" in msg
    rc, msg = refused(valid(s_labels=B - 1))
    assert rc == INV and b"s_labels" in msg
    rc, msg = refused(valid(cursor=None))                        # advance without a cursor
    assert rc == INV and b"advance needs a cursor" in msg
    for adv in (2, -1):
        rc, msg = refused(valid(advance=adv))
        assert rc == INV and b"advance must be 0 or 1" in msg
    rc, msg = refused(valid(n_agents=1 << 26, s_index=0))        # 2^32 destination rows
    assert rc == INV and b"2^31" in msg


def test_overlap_refusals():
    from distributed_learning_amd import _lib
    INV = _lib.DL_ERR_INVALID
    sam_bytes = ((M - 1) * DIM + DIM) * 4
    data_bytes = ((N - 1) * B * DIM + B * DIM) * 4
    idx_bytes = N * S * B * 4
    cases = [
        (dict(data=SAMPLES), b"data overlaps samples"),
        (dict(data=SAMPLES + sam_bytes - 16), b"data overlaps samples"),
        (dict(samples=DATA + data_bytes - 16), b"data overlaps samples"),
        (dict(data=TARGETS + 16), b"data overlaps targets"),
        (dict(data=INDEX + idx_bytes - 16), b"data overlaps index"),
        (dict(labels=SAMPLES + 1024), b"labels overlaps samples"),
        (dict(labels=TARGETS + (M - 1) * 4), b"labels overlaps targets"),
        (dict(labels=INDEX), b"labels overlaps index"),
        (dict(cursor=SAMPLES + 64), b"cursor overlaps samples"),
        (dict(cursor=TARGETS), b"cursor overlaps targets"),
        (dict(cursor=INDEX + idx_bytes - 4), b"cursor overlaps index"),
        (dict(labels=DATA + 4096), b"data overlaps labels"),
        (dict(cursor=DATA + data_bytes - 4), b"data overlaps cursor"),
        (dict(cursor=LABELS + 4), b"labels overlaps cursor"),
    ]
    for kw, text in cases:
        rc, msg = refused(valid(**kw))
        assert rc == INV and text in msg, (kw, msg)
    # touching is no overlap: the first byte after an operand is free (checked by the host
    # program below with the same extents); a shared index ends after one list
    rc, msg = refused(valid(s_index=0, cursor=INDEX + S * B * 4 - 4))
    assert rc == INV and b"cursor overlaps index" in msg


CHECK_CPP = r"""
// shape_batch_gather alone (csrc/launch.cpp + plan.cpp, no HIP, no library)
#include <cstdio>
#include <cstring>
#include "launch.h"
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
static dl_batch_gather_args valid() {
    dl_batch_gather_args a;
    std::memset(&a, 0, sizeof a);
    a.samples = (const float *)(1ull << 32); a.ld_samples = 784;
    a.targets = (const int32_t *)(1ull << 40); a.n_samples = 60000; a.dim = 784;
    a.index = (const int32_t *)(1ull << 41); a.s_index = 5 * 64;
    a.n_agents = 256; a.batch = 64; a.steps = 5;
    a.cursor = (int32_t *)(1ull << 42); a.step = 0; a.advance = 1;
    a.data = (float *)(1ull << 43); a.s_data = 64 * 784;
    a.labels = (int32_t *)(1ull << 44); a.s_labels = 64;
    return a;
}
int main() {
    char err[dl::kErrLen];
    dl::BatchGatherPlan p;
    dl_batch_gather_args a = valid();
    // the c3 shape: one wave per 784-float row, 4 rows a pass, 4096 passes on 256 CUs x 16 waves
    EXPECT(dl::shape_batch_gather(&a, 256, &p, err) == DL_OK);
    EXPECT(p.wide == 1 && p.wave_rows == 4 && p.grid == 1024 && p.k.dim4 == 196);
    EXPECT(p.k.rows == 256 * 64 && p.k.lane_sh == 6 && p.k.cursor == a.cursor);
    EXPECT(dl::shape_batch_gather(&a, 256, nullptr, err) == DL_OK);   // the check alone
    a.n_agents = 3;                       // 192 rows: 48 passes, 12 workgroups of four waves
    EXPECT(dl::shape_batch_gather(&a, 256, &p, err) == DL_OK && p.grid == 12);
    a.n_agents = 1; a.batch = 1; a.s_data = 784; a.s_labels = 1; a.s_index = 0;
    EXPECT(dl::shape_batch_gather(&a, 256, &p, err) == DL_OK && p.grid == 1);
    EXPECT(dl::shape_batch_gather(&a, 0, &p, err) == DL_OK && p.grid == 1);
    // rows shorter than a wave-instruction are packed: dim 12 -> 4 lanes a row, 16 rows an
    // instruction, 64 a pass; dim 252 -> all 64 lanes (63 used); dim 256 is wide
    a = valid(); a.dim = 12; a.ld_samples = 16; a.s_data = 64 * 12;
    EXPECT(dl::shape_batch_gather(&a, 256, &p, err) == DL_OK);
    EXPECT(p.wide == 0 && p.k.lane_sh == 2 && p.wave_rows == 64 && p.grid == 64 && p.k.dim4 == 3);
    a.dim = 4; a.s_data = 64 * 4;
    EXPECT(dl::shape_batch_gather(&a, 256, &p, err) == DL_OK && p.k.lane_sh == 0 &&
           p.wave_rows == 256 && p.grid == 16);
    a.dim = 252; a.ld_samples = 252; a.s_data = 64 * 252;
    EXPECT(dl::shape_batch_gather(&a, 256, &p, err) == DL_OK && p.wide == 0 && p.k.lane_sh == 6 &&
           p.wave_rows == 4);
    a.dim = 256; a.ld_samples = 256; a.s_data = 64 * 256;
    EXPECT(dl::shape_batch_gather(&a, 256, &p, err) == DL_OK && p.wide == 1);
    // nullable operands, host step (any sign, taken mod steps), shared index, padded strides
    a = valid(); a.labels = nullptr; a.targets = nullptr;
    EXPECT(dl::shape_batch_gather(&a, 256, &p, err) == DL_OK && !p.k.labels);
    a = valid(); a.cursor = nullptr; a.advance = 0; a.step = 12;
    EXPECT(dl::shape_batch_gather(&a, 256, &p, err) == DL_OK && p.k.step == 2 && !p.k.cursor);
    a.step = -1;
    EXPECT(dl::shape_batch_gather(&a, 256, &p, err) == DL_OK && p.k.step == 4);
    a = valid(); a.s_index = 0; a.s_data = 64 * 784 + 8; a.s_labels = 100; a.ld_samples = 1024;
    EXPECT(dl::shape_batch_gather(&a, 256, &p, err) == DL_OK);
    // a dataset past 4 GiB
    a = valid(); a.n_samples = (1 << 20) + 8; a.dim = 1024; a.ld_samples = 1024;
    a.s_data = 64 * 1024; a.targets = (const int32_t *)(1ull << 45);
    EXPECT(dl::shape_batch_gather(&a, 256, &p, err) == DL_OK);
    // touching operands do not overlap; one byte further they do
    a = valid();
    const size_t sam = ((size_t)(a.n_samples - 1) * a.ld_samples + a.dim) * 4;
    a.data = (float *)((const char *)a.samples + sam);
    EXPECT(dl::shape_batch_gather(&a, 256, &p, err) == DL_OK);
    a.data = (float *)((const char *)a.samples + sam - 16);
    EXPECT(dl::shape_batch_gather(&a, 256, &p, err) == DL_ERR_INVALID &&
           std::strstr(err, "data overlaps samples"));
    a = valid(); a.advance = 1; a.cursor = nullptr;
    EXPECT(dl::shape_batch_gather(&a, 256, &p, err) == DL_ERR_INVALID &&
           std::strstr(err, "advance needs a cursor"));
    EXPECT(dl::shape_batch_gather(nullptr, 256, &p, err) == DL_ERR_INVALID);
    std::printf("%d failures\n", fails);
    return fails != 0;
}
"""


def test_sanitized_checker_accepts_valid_shapes(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++", path="/opt/rocm/llvm/bin")
    if not cxx:
        pytest.skip("no host C++ compiler (g++ or the ROCm clang++)")
    src = tmp_path / "batch_gather_check.cpp"
    src.write_text(CHECK_CPP)
    exe = str(tmp_path / "batch_gather_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    str(src), os.path.join(CSRC, "launch.cpp"), os.path.join(CSRC, "plan.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr[:4000]
    assert run.stdout.split() == ["0", "failures"]
