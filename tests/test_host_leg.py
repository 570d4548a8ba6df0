"""The host <-> HBM leg (csrc/hostleg.hip): pinned memory, asynchronous copies ordered by events, the landing kernel, the file
loaders, and their Node side.  CPU tests read the header, the library, the addon and the cross-compiled ISA; GPU tests are bit-exact
against numpy restatements and against pil2gl.io.load_pols / save_pols."""
import ctypes as C
import filecmp
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, P, rand_field

pil2gl = pytest.importorskip("pil2gl")
from pil2gl import _lib, io  # noqa: E402

NODE = shutil.which("node")
PKG = os.path.join(ROOT, "pil2-stark-js_amd")
NEW_SYMBOLS = ["pil2gl_host_alloc", "pil2gl_host_free", "pil2gl_host_register", "pil2gl_host_unregister", "pil2gl_dev_upload_async",
               "pil2gl_dev_download_async", "pil2gl_copy_after", "pil2gl_copy_fence", "pil2gl_copy_sync", "pil2gl_land_rows_dev",
               "pil2gl_dev_load_file", "pil2gl_dev_save_file"]
NO_BAD = 0xFFFFFFFFFFFFFFFF
EINVAL = -1


# ---- CPU -------------------------------------------------------------------------------------------------------------------

def test_host_leg_symbols_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pil2gl.h")).read(), flags=re.S)
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, header), n + " is not declared in pil2gl.h"
        assert hasattr(lib, n), "libpil2gl.so does not export " + n
        assert n in _lib.SIGNATURES, n + " is not bound in _lib.py"
    assert callable(io.load_pols_dev) and callable(io.save_pols_dev)


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_addon_and_js_export_the_host_leg():
    js = ("const m=require(%r);const n=require(%r);const a=m.native;"
          "for (const k of ['hostAlloc','hostFree','hostRegister','hostUnregister','devUploadAsync','devDownloadAsync','copyAfter','copyFence',"
          "'copySync','landRowsDev','devLoadFile','devSaveFile']) if (typeof a[k] !== 'function') throw new Error('missing '+k);"
          "for (const k of ['PinnedBuffer','copyAfter','copyFence','copySync']) if (typeof m[k] !== 'function' || m[k] !== n[k]) throw new Error('missing '+k);"
          "for (const k of ['fromHost','fromFile']) if (typeof m.DevBuffer[k] !== 'function') throw new Error('missing DevBuffer.'+k);"
          "for (const k of ['uploadAsync','downloadAsync','toFile']) if (typeof m.DevBuffer.prototype[k] !== 'function') throw new Error('missing '+k);"
          "for (const k of ['length','getElement','setElement','slice','set','free']) if (!(k === 'length' || typeof m.PinnedBuffer.prototype[k] === 'function')) throw new Error('PinnedBuffer.'+k);"
          "console.log('ok')") % (os.path.join(PKG, "js", "index.js"), os.path.join(PKG, "js", "native.js"))
    out = subprocess.run([NODE, "-e", js], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr


def test_landing_kernel_isa_is_vectorised_and_spills_nothing(tmp_path):
    """every form of land_rows_kernel that the addresses allow 16-byte access for -- the in-place check (loads), the equal-width copy and
    the even-width widening (loads and stores) -- has them in the gfx950 ISA, and no form uses scratch"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path / "hostleg.s"
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "-ffp-contract=off", "-I" + os.path.join(PKG, "build"),
                           "-S", "--cuda-device-only", os.path.join(PKG, "csrc", "hostleg.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    isa = out.read_text()
    bodies = {}
    for m in re.finditer(r"^(_Z\w*land_rows_kernel\w*):[^\n]*\n(.*?)^\.Lfunc_end", isa, flags=re.S | re.M):
        mode = int(re.search(r"land_rows_kernelILi(\d+)E", m.group(1)).group(1))
        bodies[mode] = m.group(2)
    assert sorted(bodies) == [0, 1, 2, 3], sorted(bodies)          # LAND_CHECK, LAND_COPY, LAND_WIDE2, LAND_WORD
    assert "global_load_dwordx4" in bodies[0]
    for mode in (1, 2):
        assert "global_load_dwordx4" in bodies[mode] and "global_store_dwordx4" in bodies[mode], mode
    scratch = re.findall(r"^; ScratchSize: (\d+)", isa, flags=re.M)
    assert len(scratch) >= 4 and all(int(s) == 0 for s in scratch), scratch
    assert "scratch_" not in "".join(bodies.values())


# ---- GPU -------------------------------------------------------------------------------------------------------------------

def _torch():
    import torch
    pil2gl.init(0)
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _field_mix(rng, n):
    """words drawn from {0, 1, p - 1, random canonical}"""
    a = rand_field(rng, n)
    pick = rng.integers(0, 8, size=n)
    a[pick == 0] = 0
    a[pick == 1] = 1
    a[pick == 2] = P - 1
    return a


def _land_expected(a, rows, sc, dc):
    e = np.zeros((rows, dc), dtype=np.uint64)
    e[:, :sc] = a.reshape(rows, sc)
    bad = a >= np.uint64(P)
    return e.reshape(-1), (int(np.argmax(bad)) if bad.any() else NO_BAD)


def _land(torch, lib, a, rows, sc, dc, s_off, d_off, in_place=False):
    """a (rows*sc words) placed s_off words into a 16-byte aligned device buffer, landed d_off words into another one (or onto itself);
    -> (landed words, first bad index); the guard words around the destination must come back untouched"""
    GUARD = 0xA5A5A5A5A5A5A5A5
    src = torch.zeros(a.size + 4, dtype=torch.int64, device="cuda")
    src[s_off:s_off + a.size] = _dev(torch, a)
    assert src.data_ptr() % 16 == 0
    n_out = rows * dc
    if in_place:
        dst, d_off = src, s_off
    else:
        dst = _dev(torch, np.full(n_out + 4, GUARD, dtype=np.uint64))
    torch.cuda.synchronize()
    bad = C.c_uint64(12345)
    rc = lib.pil2gl_land_rows_dev(src.data_ptr() + 8 * s_off, sc, dst.data_ptr() + 8 * d_off, dc, rows, C.byref(bad), None)
    assert rc == 0, lib.pil2gl_last_error()
    out = _host(dst)
    if not in_place:
        assert (out[:d_off] == GUARD).all() and (out[d_off + n_out:] == GUARD).all(), "the landing pass wrote outside its destination"
    return out[d_off:d_off + n_out], bad.value


WIDTHS = [(6, 6), (7, 7), (7, 10), (6, 9), (1, 5), (100, 128)]     # equal (even, odd) / odd -> even / even -> odd / 1 -> 5 / 100 -> 128


@pytest.mark.gpu
@pytest.mark.parametrize("sc,dc", WIDTHS)
def test_land_rows_matches_numpy(sc, dc):
    torch, lib = _torch(), _lib.load()
    rng = np.random.default_rng(sc * 1000 + dc)
    for rows in (0, 1, 3, (1 << 16) // sc + 3):                     # the last one crosses 2^16 words
        a = _field_mix(rng, rows * sc)
        want, _ = _land_expected(a, rows, sc, dc)
        for s_off, d_off in ((0, 0), (1, 1), (1, 0), (0, 1)):       # (1, 1): both one word off a 16-byte boundary
            got, bad = _land(torch, lib, a, rows, sc, dc, s_off, d_off)
            assert (got == want).all(), (rows, s_off, d_off)
            assert bad == NO_BAD, (rows, s_off, d_off, bad)
        if sc == dc:
            for s_off in (0, 1):
                got, bad = _land(torch, lib, a, rows, sc, dc, s_off, s_off, in_place=True)
                assert (got == want).all() and bad == NO_BAD, (rows, s_off)


@pytest.mark.gpu
@pytest.mark.parametrize("sc,dc", WIDTHS)
def test_land_rows_reports_the_first_non_canonical_word(sc, dc):
    torch, lib = _torch(), _lib.load()
    rng = np.random.default_rng(sc * 77 + dc)
    rows = (1 << 16) // sc + 3
    n = rows * sc
    base = _field_mix(rng, n)
    # first word, last word, either side of the 256 and 512 words a workgroup's first pass spans (one word or one pair per thread)
    spots = [0, n - 1, 255, 256, 511, 512, 513, n // 2]
    for k, at in enumerate(spots):
        for v in (P, P + 1, 2 ** 64 - 1):
            a = base.copy(); a[at] = v
            want, first = _land_expected(a, rows, sc, dc)
            assert first == at
            for s_off, d_off in ((0, 0), (1, 1)) if k % 2 == 0 else ((1, 0),):
                got, bad = _land(torch, lib, a, rows, sc, dc, s_off, d_off)
                assert bad == at, (at, v, s_off, d_off, bad)
                assert (got == want).all()                           # the data is landed all the same
            if sc == dc:
                got, bad = _land(torch, lib, a, rows, sc, dc, 1, 1, in_place=True)
                assert bad == at and (got == want).all()
    for lo, hi in ((0, n - 1), (255, 256), (511, 40000), (512, 513), (n - 2, n - 1), (300, 60000)):
        a = base.copy(); a[hi] = P; a[lo] = 2 ** 64 - 1
        _, first = _land_expected(a, rows, sc, dc)
        assert first == lo
        for s_off, d_off in ((0, 0), (1, 1)):
            assert _land(torch, lib, a, rows, sc, dc, s_off, d_off)[1] == lo, (lo, hi)
    # narrowing is an error, not a truncation
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    assert lib.pil2gl_land_rows_dev(t.data_ptr(), 4, t.data_ptr() + 256, 3, 2, None, None) == EINVAL


CHUNK = 4096
FILE_WORDS = [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 5 * CHUNK + 3]


@pytest.mark.gpu
def test_dev_load_file_equals_load_pols(tmp_path):
    torch = _torch()
    rng = np.random.default_rng(5)
    for n in FILE_WORDS:
        a = _field_mix(rng, n)
        f = tmp_path / ("w%d.commit" % n)
        a.astype("<u8").tofile(f)
        want = io.load_pols(str(f), n, 1, device="cuda")
        got = io.load_pols_dev(str(f), n, 1, chunk_words=CHUNK)
        assert got.shape == want.shape and torch.equal(got, want), n
        # a non-zero byteOffset: the same words behind 24 bytes of something else
        g = tmp_path / ("o%d.commit" % n)
        with open(g, "wb") as fh:
            fh.write(b"\xff" * 24); fh.write(a.astype("<u8").tobytes())
        assert torch.equal(io.load_pols_dev(str(g), n, 1, chunk_words=CHUNK, byte_offset=24), want), n
    # rows widened on the way (writeToBigBuffer(buff, nCols)): chunks hold whole rows, many turns of the double buffer
    for rows, sc, dc in ((5 * CHUNK + 3, 3, 8), (2051, 100, 128), (2051, 7, 10), (1, 4096, 4097), (0, 3, 8)):
        a = _field_mix(rng, rows * sc)
        f = tmp_path / ("r%d_%d.commit" % (rows, sc))
        a.astype("<u8").tofile(f)
        want = torch.zeros(rows, dc, dtype=torch.int64, device="cuda")
        want[:, :sc] = io.load_pols(str(f), rows, sc, device="cuda").reshape(rows, sc)
        got = io.load_pols_dev(str(f), rows, sc, dst_cols=dc, chunk_words=CHUNK)
        assert torch.equal(got, want.reshape(-1)), (rows, sc, dc)
    # the default chunk (2^25 words) on a file smaller than one
    a = _field_mix(rng, 100 * 1000)
    f = tmp_path / "d.commit"
    a.astype("<u8").tofile(f)
    assert torch.equal(io.load_pols_dev(str(f), 1000, 100), io.load_pols(str(f), 1000, 100, device="cuda"))


@pytest.mark.gpu
def test_dev_load_file_checks_words_and_file_size(tmp_path):
    torch, lib = _torch(), _lib.load()
    rng = np.random.default_rng(6)
    n = 5 * CHUNK + 3
    a = _field_mix(rng, n)
    for at in (0, CHUNK - 1, CHUNK, 3 * CHUNK + 7, n - 1):
        b = a.copy(); b[at] = P + 1; b[n - 1] = max(int(b[n - 1]), P)       # a later one too (the last word), the first is reported
        f = tmp_path / "bad.commit"
        b.astype("<u8").tofile(f)
        dst = torch.zeros(n, dtype=torch.int64, device="cuda")
        bad = C.c_uint64(0)
        assert lib.pil2gl_dev_load_file(str(f).encode(), 0, n, 1, dst.data_ptr(), 1, CHUNK, C.byref(bad)) == 0
        assert bad.value == at and (_host(dst) == b).all()              # landed all the same
        with pytest.raises(ValueError) as e:
            io.load_pols_dev(str(f), n, 1, chunk_words=CHUNK)
        assert "bad.commit" in str(e.value) and "word %d " % at in str(e.value) and str(int(b[at])) in str(e.value)
        # widened: the index is still the word's place in the file
        rows = n // 3
        wide = torch.zeros(rows * 4, dtype=torch.int64, device="cuda")
        assert lib.pil2gl_dev_load_file(str(f).encode(), 0, rows, 3, wide.data_ptr(), 4, CHUNK, C.byref(bad)) == 0
        assert bad.value == (at if at < rows * 3 else NO_BAD)
    # one byte short: PIL2GL_EINVAL with file, found and expected size; nothing is copied, nothing faults
    f = tmp_path / "short.commit"
    with open(f, "wb") as fh:
        fh.write(a.astype("<u8").tobytes()[:-1])
    dst = torch.full((n,), 7, dtype=torch.int64, device="cuda")
    for off, rows in ((0, n), (8, n - 1)):
        assert lib.pil2gl_dev_load_file(str(f).encode(), off, rows, 1, dst.data_ptr(), 1, CHUNK, None) == EINVAL
        msg = lib.pil2gl_last_error().decode()
        assert "short.commit" in msg and str(8 * n - 1) in msg and str(8 * n) in msg, msg
    assert (dst == 7).all()
    assert lib.pil2gl_dev_load_file(str(tmp_path / "missing.commit").encode(), 0, 1, 1, dst.data_ptr(), 1, CHUNK, None) == EINVAL
    assert lib.pil2gl_dev_load_file(str(f).encode(), 0, 4, 4, dst.data_ptr(), 3, CHUNK, None) == EINVAL               # narrowing


@pytest.mark.gpu
def test_dev_save_file_equals_save_pols(tmp_path):
    torch = _torch()
    rng = np.random.default_rng(7)
    for n in FILE_WORDS:
        t = _dev(torch, _field_mix(rng, n))
        f1, f2 = tmp_path / ("a%d" % n), tmp_path / ("b%d" % n)
        io.save_pols(t, str(f1))
        f2.write_bytes(b"stale contents that are longer than nothing" * 3)          # an older file of the same name is replaced
        io.save_pols_dev(t, str(f2), chunk_words=CHUNK)
        assert filecmp.cmp(str(f1), str(f2), shallow=False), n
        # behind a header
        f3 = tmp_path / ("c%d" % n)
        f3.write_bytes(b"\x01" * 16)
        io.save_pols_dev(t, str(f3), chunk_words=CHUNK, byte_offset=16)
        assert f3.read_bytes() == b"\x01" * 16 + f1.read_bytes(), n
    t = _dev(torch, _field_mix(rng, 70000))
    io.save_pols(t, str(tmp_path / "d1")); io.save_pols_dev(t, str(tmp_path / "d2"))       # default chunk
    assert filecmp.cmp(str(tmp_path / "d1"), str(tmp_path / "d2"), shallow=False)
    assert torch.equal(io.load_pols_dev(str(tmp_path / "d2"), 70000, 1), t)


def _pinned(lib, n):
    p = C.c_void_p()
    assert lib.pil2gl_host_alloc(n, C.byref(p)) == 0, lib.pil2gl_last_error()
    return p, np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(n,))


@pytest.mark.gpu
def test_async_upload_is_ordered_by_copy_after_and_copy_fence():
    """a running sequence of trees reads a device buffer on a user stream; the upload of new contents is placed after it with
    copy_after, and the next tree after the upload with copy_fence: trees enqueued before see the OLD words, the one after the NEW"""
    torch, lib = _torch(), _lib.load()
    width, height = 16, 1 << 20
    n = width * height                                                     # 2^24 words
    rng = np.random.default_rng(8)
    old, new = rand_field(rng, n), rand_field(rng, n)
    n_nodes = lib.pil2gl_merkle_num_nodes(height)
    d = _dev(torch, old)
    ref = []                                                                # the two trees from buffers nothing else touches
    for a in (old, new):
        t, nodes = _dev(torch, a), torch.zeros(n_nodes, dtype=torch.int64, device="cuda")
        assert lib.pil2gl_merkelize_dev(t.data_ptr(), width, height, 0, nodes.data_ptr(), None) == 0
        torch.cuda.synchronize()
        ref.append(_host(nodes).copy())
    assert not (ref[0][-4:] == ref[1][-4:]).all()
    ptr, h = _pinned(lib, n)
    try:
        h[:] = new
        s = torch.cuda.Stream()
        before = [torch.zeros(n_nodes, dtype=torch.int64, device="cuda") for _ in range(6)]
        after = torch.zeros(n_nodes, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for nodes in before:                                                # ~ milliseconds of queued work that reads d
            assert lib.pil2gl_merkelize_dev(d.data_ptr(), width, height, 0, nodes.data_ptr(), s.cuda_stream) == 0
        assert lib.pil2gl_copy_after(s.cuda_stream) == 0                    # the upload must not overtake those readers
        assert lib.pil2gl_dev_upload_async(d.data_ptr(), ptr, n) == 0
        assert lib.pil2gl_copy_fence(s.cuda_stream) == 0                    # and the next reader waits for it
        assert lib.pil2gl_merkelize_dev(d.data_ptr(), width, height, 0, after.data_ptr(), s.cuda_stream) == 0
        s.synchronize()
        for nodes in before:
            assert (_host(nodes) == ref[0]).all(), "a tree enqueued before the upload saw new words"
        assert (_host(after) == ref[1]).all(), "the tree enqueued after the fence saw old words"
        # and back: download_async after the stream's work, host waits with copy_sync
        h[:] = 0
        assert lib.pil2gl_copy_after(s.cuda_stream) == 0
        assert lib.pil2gl_dev_download_async(ptr, d.data_ptr(), n) == 0
        assert lib.pil2gl_copy_sync() == 0
        assert (h == new).all()
    finally:
        assert lib.pil2gl_host_free(ptr) == 0


@pytest.mark.gpu
def test_async_copies_refuse_pageable_memory_and_survive_shutdown(tmp_path):
    torch, lib = _torch(), _lib.load()
    n = 1 << 16
    a = rand_field(np.random.default_rng(9), n)
    back = np.zeros(n, dtype=np.uint64)
    d = torch.zeros(n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for host in (a, back):
        assert lib.pil2gl_dev_upload_async(d.data_ptr(), host.ctypes.data, n) == EINVAL     # never a silent synchronous copy
        assert "pinned" in lib.pil2gl_last_error().decode()
        assert lib.pil2gl_dev_download_async(host.ctypes.data, d.data_ptr(), n) == EINVAL
    assert (_host(d) == 0).all() and (back == 0).all()
    assert lib.pil2gl_host_register(a.ctypes.data, n) == 0, lib.pil2gl_last_error()
    assert lib.pil2gl_host_register(back.ctypes.data, n) == 0, lib.pil2gl_last_error()
    try:
        assert lib.pil2gl_dev_upload_async(d.data_ptr(), a.ctypes.data, n) == 0, lib.pil2gl_last_error()
        assert lib.pil2gl_dev_download_async(back.ctypes.data, d.data_ptr(), n) == 0          # same stream: after the upload
        assert lib.pil2gl_copy_sync() == 0
        assert (back == a).all() and (_host(d) == a).all()
    finally:
        assert lib.pil2gl_host_unregister(a.ctypes.data) == 0
        assert lib.pil2gl_host_unregister(back.ctypes.data) == 0
    assert lib.pil2gl_dev_upload_async(d.data_ptr(), a.ctypes.data, n) == EINVAL             # pageable again
    # shutdown destroys the stream, the events and the pinned chunks; the next call builds them again
    f = tmp_path / "s.commit"
    a.astype("<u8").tofile(f)
    assert torch.equal(io.load_pols_dev(str(f), n, 1, chunk_words=CHUNK), _dev(torch, a))
    pil2gl.shutdown(); pil2gl.init(0)
    assert torch.equal(io.load_pols_dev(str(f), n, 1, chunk_words=CHUNK), _dev(torch, a))
    ptr, h = _pinned(lib, n)
    h[:] = a
    d.zero_(); torch.cuda.synchronize()
    assert lib.pil2gl_dev_upload_async(d.data_ptr(), ptr, n) == 0 and lib.pil2gl_copy_sync() == 0
    assert (_host(d) == a).all()
    assert lib.pil2gl_host_free(ptr) == 0


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_consttree_read_into_hbm_and_pinned_buffer_from_node(tmp_path):
    """tests/js/host_leg.js: trees written by writeToFile (GL plain and split, BN128 arity 4 custom and arity 16) read back with
    {device: true}: same root, same group proofs as the host-read tree; PinnedBuffer answers BigBuffer's calls across chunk
    boundaries (for the elements of either family too), and its memory survives free / allocate / collect cycles; DevBuffer.fromFile /
    toFile / fromHost round trips, toFile of words an enqueue-only call has just produced, and the canonicity error"""
    out = subprocess.run([NODE, "--expose-gc", os.path.join(ROOT, "tests", "js", "host_leg.js"), str(tmp_path)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "host leg OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def _canon(v):          # canonical text of a proof (= tests/js/prove_c3.js)
    if isinstance(v, dict):
        return "{" + ",".join('"%s":%s' % (k, _canon(x)) for k, x in v.items()) + "}"
    if isinstance(v, (list, tuple)):
        return "[" + ",".join(_canon(x) for x in v) + "]"
    return '"%d"' % int(v)


def _prove_from_host(tmp_path, n_bits, n_cols, steps, n_queries, proofs, from_file):
    """two witnesses proved by the Python-driven prover (the digests to meet), then tests/js/prove_from_host.js proves them alternately
    from pinned host memory with the next upload under the running proof -> (its JSON line, the digest each proof must have)"""
    import hashlib
    import torch
    import bench
    from pil2gl import stark
    ss = {"nBits": n_bits, "nBitsExt": n_bits + 3, "nQueries": n_queries, "verificationHashType": "GL", "splitLinearHash": False,
          "steps": [{"nBits": b} for b in steps]}
    info, exprs, _ = stark.fibonacci_air(n_cols // 2, ss)
    gpu = stark.GpuBackend(0, False)
    dev = torch.device("cuda", 0)
    witnesses, const_root = [], None
    for seed in (0, 1):
        cm, consts, publics = bench.fibonacci_trace_gpu(dev, n_bits, n_cols // 2, seed)
        start = [int(v) for v in cm[:n_cols].cpu().numpy().view(np.uint64)]
        setup = stark.build_const_tree(gpu, consts, info)
        res = stark.stark_gen(gpu, cm, setup, info, exprs, publics)
        torch.cuda.synchronize()
        witnesses.append({"start": [str(v) for v in start], "publics": [str(v) for v in publics], "queries": res["queries"],
                          "proofSha256": hashlib.sha256(_canon(res["proof"]).encode()).hexdigest()})
        const_root = [str(v) for v in setup["constRoot"]]
        del cm, setup, res
    assert witnesses[0]["proofSha256"] != witnesses[1]["proofSha256"]
    torch.cuda.empty_cache()
    job = {"pilInfo": info, "expressionsInfo": exprs, "constRoot": const_root, "witnesses": witnesses, "proofs": proofs,
           "commitDir": str(tmp_path) if from_file else None}
    f = tmp_path / "job.json"
    f.write_text(json.dumps(job))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "prove_from_host.js"), str(f)], capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0 and "prove from host OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    return line, [witnesses[k % 2]["proofSha256"] for k in range(proofs)]


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_proofs_from_host_witnesses_2e18(tmp_path):
    """2^18 x 20, two witnesses alternating, each read from a `.commit` file into a PinnedBuffer and uploaded under the proof before it:
    every proof's digest is the Python-driven digest of ITS witness (a stale or half-uploaded buffer cannot give it)"""
    line, want = _prove_from_host(tmp_path, 18, 20, (21, 16, 11, 6), 32, 5, True)
    print(json.dumps(line))
    assert line["proofSha256"] == want


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_config3_node_proofs_from_host_witnesses(tmp_path):
    """BASELINE config 3 (2^24 x 100) from two pinned 13.4 GB host witnesses: digests as above; the upload of witness k + 1 is hidden
    under proof k (steady state within 10 % of the same proof from a resident witness, the margin test_config3_proof_driven_from_node
    grants a Node-driven proof), pinned asynchronous upload beats the pageable pil2gl_dev_upload, and the landing pass costs under 5 % of
    the upload rate.  The figures go to profiles/host_leg_config3.json when PIL2GL_WRITE_PROFILES is set.
    Measured on an MI355X: see LAB_NOTES.md, "Host leg"."""
    import torch
    if torch.cuda.mem_get_info()[0] < 230e9:
        pytest.skip("needs ~230 GB of free device memory")
    line, want = _prove_from_host(tmp_path, 24, 100, (27, 22, 17, 12, 7), 64, 5, False)
    print("config 3 from host:", json.dumps({k: v for k, v in line.items() if k != "proofSha256"}))
    if os.environ.get("PIL2GL_WRITE_PROFILES"):
        with open(os.path.join(ROOT, "profiles", "host_leg_config3.json"), "w") as fh:
            json.dump(line, fh, indent=1)
    assert line["proofSha256"] == want
    assert line["steady_seconds"] <= 1.10 * line["resident_seconds"], (line["steady_seconds"], line["resident_seconds"])
    assert line["h2d_GBps"] > line["h2d_pageable_GBps"], (line["h2d_GBps"], line["h2d_pageable_GBps"])
    assert line["h2d_landed_GBps"] >= 0.95 * line["h2d_GBps"], (line["h2d_landed_GBps"], line["h2d_GBps"])
