"""CPU checks of dl_image_batch's C ABI: the struct layout agrees between C and ctypes, the symbol
is additive (ABI still 10), every refusal the header states comes back with its status and its
own message before any device call (dummy pointers, runs without a GPU), and the host-only
checker (csrc/launch.cpp shape_image_batch) accepts the valid call shapes and shapes their
launches -- the latter from a small stand-alone program built with the address and
undefined-behaviour sanitizers and run as an ordinary process."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-learning_amd", "csrc")

FIELDS = ["samples", "ld_samples", "targets", "n_samples", "channels", "height", "width", "lut",
          "index", "s_index", "aug", "s_aug", "pad", "fill", "n_agents", "batch", "steps",
          "cursor", "step", "advance", "data", "s_data", "labels", "s_labels"]


def test_struct_layout_matches_c(tmp_path):
    from distributed_learning_amd import _lib
    offs = "".join(f'printf("%zu ", offsetof(dl_image_batch_args, {f}));' for f in FIELDS)
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dlamd.h"\n'
                    'int main(void){printf("%zu ", sizeof(dl_image_batch_args));' + offs +
                    'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)],
                   check=True)
    c = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                        check=True).stdout.split()]
    A = _lib.DlImageBatchArgs
    assert [f for f, _ in A._fields_] == FIELDS
    assert c == [ctypes.sizeof(A)] + [getattr(A, f).offset for f in FIELDS]


def test_symbol_is_additive():
    from distributed_learning_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "dl_image_batch")
    assert "dl_image_batch" in _lib.SIGNATURES
    assert lib.dl_abi_version() == 10 == _lib.ABI_VERSION


# dummy device addresses, never dereferenced, far apart
SAMPLES, TARGETS, INDEX, CURSOR, DATA, LABELS, AUG, LUT = (1 << 32, 1 << 40, 1 << 41, 1 << 42,
                                                           1 << 43, 1 << 44, 1 << 45, 1 << 46)
M, C, H, W, N, B, S, PAD = 50000, 3, 32, 32, 8, 64, 5, 4
D = C * H * W


def valid(**kw):
    from distributed_learning_amd import _lib
    a = _lib.DlImageBatchArgs(SAMPLES, D, TARGETS, M, C, H, W, LUT, INDEX, S * B, AUG, S * B,
                              PAD, 0, N, B, S, CURSOR, 0, 1, DATA, B * D, LABELS, B)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def refused(a):
    """(status, message) of a call that must be refused before any device call."""
    from distributed_learning_amd import _lib
    lib = _lib.load()
    rc = lib.dl_image_batch(ctypes.byref(a) if a is not None else None, None)
    return rc, lib.dl_last_error()


def test_refusals():
    from distributed_learning_amd import _lib
    INV = _lib.DL_ERR_INVALID
    rc, msg = refused(None)
    assert rc == INV and b"args is NULL" in msg
    for f in ("samples", "index", "data", "lut"):
        rc, msg = refused(valid(**{f: None}))
        assert rc == INV and b"null samples, index, data or lut" in msg, (f, msg)
    for f in ("n_agents", "batch", "steps", "n_samples"):
        for v in (0, -1):
            rc, msg = refused(valid(**{f: v}))
            assert rc == INV and b"n_samples must be >= 1" in msg, (f, v, msg)
    for f in ("height", "width"):
        for v in (0, -4):
            rc, msg = refused(valid(**{f: v}))
            assert rc == INV and b"height and width must be >= 1" in msg, (f, v, msg)
    for c in (0, -1, 17):
        rc, msg = refused(valid(channels=c))
        assert rc == INV and b"channels must lie in [1, 16]" in msg, (c, msg)
    for w in (30, 33, 1, 2):
        rc, msg = refused(valid(width=w))
        assert rc == INV and b"width must be a multiple of 4" in msg, (w, msg)
    big = dict(ld_samples=1 << 40, s_data=1 << 50, n_agents=1, batch=1, s_index=0, s_aug=0)
    for c, h, w in ((1, (1 << 14) + 1, 1 << 14), (16, 1 << 12, (1 << 12) + 4),
                    (1, (1 << 31) - 1, (1 << 31) - 4)):
        rc, msg = refused(valid(channels=c, height=h, width=w, **big))
        assert rc == INV and b"at most 2^28" in msg, (c, h, w, msg)
    for p in (-1, 128):
        rc, msg = refused(valid(pad=p))
        assert rc == INV and b"pad must lie in [0, 127]" in msg, (p, msg)
    for f in (-1, 256):
        rc, msg = refused(valid(fill=f))
        assert rc == INV and b"fill must lie in [0, 255]" in msg, (f, msg)
    for off in (1, 2, 3):
        rc, msg = refused(valid(samples=SAMPLES + off))
        assert rc == INV and b"samples must be 4-byte aligned" in msg, (off, msg)
    for ld in (D - 4, D + 2, 0):
        rc, msg = refused(valid(ld_samples=ld))
        assert rc == INV and b"ld_samples" in msg, (ld, msg)
    rc, msg = refused(valid(data=DATA + 8))
    assert rc == INV and b"data and lut must be 16-byte aligned" in msg
    rc, msg = refused(valid(lut=LUT + 4))
    assert rc == INV and b"data and lut must be 16-byte aligned" in msg
    for sd in (B * D - 4, B * D + 2, 0):
        rc, msg = refused(valid(s_data=sd))
        assert rc == INV and b"s_data" in msg, (sd, msg)
    for si in (S * B - 1, 1, -S * B):
        rc, msg = refused(valid(s_index=si))
        assert rc == INV and b"s_index" in msg, (si, msg)
        rc, msg = refused(valid(s_aug=si))
        assert rc == INV and b"s_aug" in msg, (si, msg)
    rc, msg = refused(valid(s_labels=B - 1))
    assert rc == INV and b"s_labels" in msg
    rc, msg = refused(valid(targets=None))                       # labels without targets
    assert rc == INV and b"labels need targets" in msg
    rc, msg = refused(valid(cursor=None))                        # advance without a cursor
    assert rc == INV and b"advance needs a cursor" in msg
    for adv in (2, -1):
        rc, msg = refused(valid(advance=adv))
        assert rc == INV and b"advance must be 0 or 1" in msg
    rc, msg = refused(valid(n_agents=1 << 26, s_index=0, s_aug=0))   # 2^32 destination images
    assert rc == INV and b"2^31" in msg


def test_overlap_refusals():
    from distributed_learning_amd import _lib
    INV = _lib.DL_ERR_INVALID
    sam_bytes = (M - 1) * D + D
    data_bytes = ((N - 1) * B * D + B * D) * 4
    idx_bytes = N * S * B * 4
    lut_bytes = C * 256 * 4
    cases = [
        (dict(data=SAMPLES), b"data overlaps samples"),
        (dict(data=SAMPLES + sam_bytes - 16), b"data overlaps samples"),
        (dict(samples=DATA + data_bytes - 4), b"data overlaps samples"),
        (dict(data=TARGETS + 16), b"data overlaps targets"),
        (dict(data=INDEX + idx_bytes - 16), b"data overlaps index"),
        (dict(data=AUG + idx_bytes - 16), b"data overlaps aug"),
        (dict(data=LUT + lut_bytes - 16), b"data overlaps lut"),
        (dict(labels=SAMPLES + 1024), b"labels overlaps samples"),
        (dict(labels=TARGETS + (M - 1) * 4), b"labels overlaps targets"),
        (dict(labels=INDEX), b"labels overlaps index"),
        (dict(labels=AUG + 64), b"labels overlaps aug"),
        (dict(labels=LUT), b"labels overlaps lut"),
        (dict(cursor=SAMPLES + 64), b"cursor overlaps samples"),
        (dict(cursor=TARGETS), b"cursor overlaps targets"),
        (dict(cursor=INDEX + idx_bytes - 4), b"cursor overlaps index"),
        (dict(cursor=AUG + idx_bytes - 4), b"cursor overlaps aug"),
        (dict(cursor=LUT + lut_bytes - 4), b"cursor overlaps lut"),
        (dict(labels=DATA + 4096), b"data overlaps labels"),
        (dict(cursor=DATA + data_bytes - 4), b"data overlaps cursor"),
        (dict(cursor=LABELS + 4), b"labels overlaps cursor"),
    ]
    for kw, text in cases:
        rc, msg = refused(valid(**kw))
        assert rc == INV and text in msg, (kw, msg)
    # exact extents: a shared list ends after one agent's entries.  Touching is no overlap: the
    # first byte after an operand is free -- checked by the host program below with the same
    # extents, since a call that passes the check would go on to launch
    for f, ptr in (("s_index", INDEX), ("s_aug", AUG)):
        name = f[2:].encode()
        rc, msg = refused(valid(**{f: 0, "cursor": ptr + S * B * 4 - 4}))
        assert rc == INV and b"cursor overlaps " + name in msg


CHECK_CPP = r"""
// shape_image_batch alone (csrc/launch.cpp + plan.cpp, no HIP, no library)
#include <cstdio>
#include <cstring>
#include "launch.h"
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
static dl_image_batch_args cifar() {
    dl_image_batch_args a;
    std::memset(&a, 0, sizeof a);
    a.samples = (const uint8_t *)(1ull << 32); a.ld_samples = 3072;
    a.targets = (const int32_t *)(1ull << 40); a.n_samples = 50000;
    a.channels = 3; a.height = 32; a.width = 32;
    a.lut = (const float *)(1ull << 46);
    a.index = (const int32_t *)(1ull << 41); a.s_index = 12 * 64;
    a.aug = (const int32_t *)(1ull << 45); a.s_aug = 12 * 64;
    a.pad = 4; a.fill = 0;
    a.n_agents = 64; a.batch = 64; a.steps = 12;
    a.cursor = (int32_t *)(1ull << 42); a.step = 0; a.advance = 1;
    a.data = (float *)(1ull << 43); a.s_data = 64 * 3072;
    a.labels = (int32_t *)(1ull << 44); a.s_labels = 64;
    return a;
}
int main() {
    char err[dl::kErrLen];
    dl::ImageBatchPlan p;
    dl_image_batch_args a = cifar();
    // CIFAR (the c5 shape): 8 lanes a row, 8 rows an instruction, 32 a pass; 4096 images on
    // 256 CUs x 16 waves, one each
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_OK);
    EXPECT(p.grid == 1024 && p.lds_bytes == 3072 && p.pass_rows == 32 && p.k.lane_sh == 3);
    EXPECT(p.k.images == 4096 && p.k.cursor == a.cursor && p.k.fill4 == 0 && p.k.aug == a.aug);
    EXPECT(dl::shape_image_batch(&a, 256, nullptr, err) == DL_OK);   // the check alone
    a.fill = 0x7f;
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_OK && p.k.fill4 == 0x7f7f7f7fu);
    // MNIST (the c3 shape), the test transform: no aug, no pad
    a = cifar(); a.channels = 1; a.height = 28; a.width = 28; a.ld_samples = 784;
    a.n_samples = 60000; a.n_agents = 256; a.s_data = 64 * 784; a.aug = nullptr; a.s_aug = 0;
    a.pad = 0;
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_OK);
    EXPECT(p.grid == 1024 && p.lds_bytes == 1024 && p.k.lane_sh == 3 && p.k.images == 16384);
    EXPECT(p.k.aug == nullptr);
    // n_cus = 0 counts as one compute unit: 16 waves
    EXPECT(dl::shape_image_batch(&a, 0, &p, err) == DL_OK && p.grid == 4);
    // 1 x 1 x 4: one lane of one wave
    a = cifar(); a.channels = 1; a.height = 1; a.width = 4; a.ld_samples = 4; a.n_agents = 1;
    a.batch = 1; a.steps = 1; a.s_index = 0; a.s_aug = 0; a.s_data = 4; a.s_labels = 1;
    a.n_samples = 1; a.pad = 0;
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_OK);
    EXPECT(p.grid == 1 && p.k.lane_sh == 0 && p.pass_rows == 256 && p.lds_bytes == 1024);
    EXPECT(dl::shape_image_batch(&a, 0, &p, err) == DL_OK && p.grid == 1);
    // rows wider than a wave-instruction: 64 lanes a row, one row an instruction
    a = cifar(); a.width = 512; a.height = 2; a.ld_samples = 3072; a.s_data = 64 * 3072;
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_OK && p.k.lane_sh == 6 &&
           p.pass_rows == 4);
    // 16 channels: the whole 16 KiB table
    a = cifar(); a.channels = 16; a.height = 2; a.width = 4; a.ld_samples = 128;
    a.s_data = 64 * 128;
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_OK && p.lds_bytes == 16384);
    // a padded ld_samples, s_data and s_labels; a shared index and aug
    a = cifar(); a.ld_samples = 3072 + 16; a.s_data = 64 * 3072 + 8; a.s_labels = 100;
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_OK && p.k.ld_samples == 3088);
    a = cifar(); a.s_index = 0; a.s_aug = 0;
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_OK);
    // s_aug is not looked at without aug
    a = cifar(); a.aug = nullptr; a.s_aug = 3;
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_OK);
    // nullable operands; a host step of any sign, taken mod steps
    a = cifar(); a.labels = nullptr; a.targets = nullptr;
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_OK && !p.k.labels);
    a = cifar(); a.cursor = nullptr; a.advance = 0; a.step = 26;
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_OK && p.k.step == 2 && !p.k.cursor);
    a.step = -1;
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_OK && p.k.step == 11);
    a.step = -2147483647 - 1;
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_OK && p.k.step == 4);
    // a dataset past 4 GiB of bytes
    a = cifar(); a.n_samples = (1 << 21) + 8; a.ld_samples = 2048; a.channels = 2;
    a.s_data = 64 * 2048; a.targets = (const int32_t *)(1ull << 47);
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_OK);
    // the largest image
    a = cifar(); a.channels = 16; a.height = 1 << 12; a.width = 1 << 12; a.n_samples = 2;
    a.ld_samples = 1ll << 28; a.n_agents = 1; a.batch = 1; a.s_data = 1ll << 28;
    a.s_index = 0; a.s_aug = 0; a.data = (float *)(1ull << 50);
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_OK);
    // touching operands do not overlap; one byte further they do
    a = cifar();
    const size_t sam = (size_t)(a.n_samples - 1) * a.ld_samples + 3072;
    a.data = (float *)((const char *)a.samples + sam);
    EXPECT(((uintptr_t)a.data & 15u) == 0);
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_OK);
    a.data = (float *)((const char *)a.samples + sam - 16);
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_ERR_INVALID &&
           std::strstr(err, "data overlaps samples"));
    a = cifar();
    const size_t db = ((size_t)(a.n_agents - 1) * a.s_data + 64 * 3072) * 4;
    a.lut = (const float *)((const char *)a.data + db);
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_OK);
    a.lut = (const float *)((const char *)a.data + db - 16);
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_ERR_INVALID &&
           std::strstr(err, "data overlaps lut"));
    a = cifar(); a.cursor = (int32_t *)((const char *)a.aug - 4);
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_OK);
    a.cursor = (int32_t *)((const char *)a.aug + ((size_t)63 * a.s_aug + 12 * 64) * 4);
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_OK);
    a.cursor = (int32_t *)((const char *)a.cursor - 4);
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_ERR_INVALID &&
           std::strstr(err, "cursor overlaps aug"));
    a = cifar(); a.advance = 1; a.cursor = nullptr;
    EXPECT(dl::shape_image_batch(&a, 256, &p, err) == DL_ERR_INVALID &&
           std::strstr(err, "advance needs a cursor"));
    EXPECT(dl::shape_image_batch(nullptr, 256, &p, err) == DL_ERR_INVALID);
    std::printf("%d failures\n", fails);
    return fails != 0;
}
"""


def test_sanitized_checker_accepts_valid_shapes(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++", path="/opt/rocm/llvm/bin")
    if not cxx:
        pytest.skip("no host C++ compiler (g++ or the ROCm clang++)")
    src = tmp_path / "image_batch_check.cpp"
    src.write_text(CHECK_CPP)
    exe = str(tmp_path / "image_batch_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    str(src), os.path.join(CSRC, "launch.cpp"), os.path.join(CSRC, "plan.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stdout + run.stderr[:4000]
    assert run.stdout.split() == ["0", "failures"]
