"""The device zlib decoder (csrc/zlib_inflate.hip) and the container read side built on it (container.read_frame,
load_compressed_device, lossless_decompress_device): the same bytes as zlib.decompress and as the host run of the same
functions, the right status on malformed input, the reference artefacts decoded exactly as the mirrored host path
decodes them, round trips through the device encoder, determinism, queued calls, and the ABI's argument errors."""
import ctypes as C
import glob
import os
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
RHCCQ_E_ARG, RHCCQ_E_LIMIT = -1, -3
OK, BAD_HEADER, BAD_DATA, TRUNCATED, ADLER, CAPACITY = 0, 1, 2, 3, 4, 5


@pytest.fixture(scope="module")
def rh():
    from roibasedimagecompression_amd.ops import Rhccq
    return Rhccq(0)


def _host(b, cap):
    from roibasedimagecompression_amd import _lib
    out = (C.c_uint8 * max(cap, 1))()
    ln, st = C.c_int64(), C.c_int32()
    src = (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b if b else b"\0")
    assert _lib.load().rhccq_zlib_decompress_host(src, len(b), out, cap, C.byref(ln), C.byref(st)) == 0
    return st.value, bytes(out[:ln.value]) if st.value == OK else ln.value


def _device(rh, b, cap):
    out, length, status = rh.zlib_decompress_async(b, cap)
    ln, st = (int(v[0]) for v in rh.to_host(length, status))
    return st, (rh.to_host(out[:ln]).tobytes() if st == OK else ln)


def _payload(n, seed):
    rnd = np.random.default_rng(seed)
    small = rnd.integers(0, 6, n // 2, dtype=np.uint8).tobytes()
    return small + bytes(rnd.integers(0, 256, n // 8, dtype=np.uint8)) + b"\x07" * (n // 4) + small[: n // 8]


def _valid_corpus():
    data = _payload(300_000, 1)
    for level in range(10):
        yield f"level{level}", zlib.compress(data, level)
    for st in (zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED):
        for wbits, mem in ((9, 1), (15, 9)):
            c = zlib.compressobj(6, zlib.DEFLATED, wbits, mem, st)
            yield f"strategy{st}-{wbits}-{mem}", c.compress(data) + c.flush()
    c = zlib.compressobj(9)
    yield "flushes", (c.compress(data[:70_000]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(data[70_000:]) + c.flush(zlib.Z_FULL_FLUSH)
                      + c.compress(b"tail") + c.flush())
    for n in (0, 1, 32767, 32768, 65535, 65536, 65537):
        yield f"size{n}", zlib.compress(data[:n], 6)
    yield "random", zlib.compress(np.random.default_rng(2).integers(0, 256, 200_000, dtype=np.uint8).tobytes(), 9)
    yield "zeros", zlib.compress(bytes(4_000_000), 9)
    inner = zlib.compress(data, 9)
    yield "stored-of-deflate", zlib.compress(inner * 3, 0)
    yield "trailing", zlib.compress(data, 9) + b"junk after the trailer"


def test_device_matches_zlib_and_host(rh):
    for name, z in _valid_corpus():
        want = zlib.decompress(z)
        cap = len(want) + 17
        assert _device(rh, z, cap) == (OK, want), name
        assert _host(z, cap) == (OK, want), name
        assert rh.to_host(rh.zlib_decompress(z)).tobytes() == want, name


def _malformed():
    z = zlib.compress(_payload(60_000, 4), 9)
    yield "empty", b""
    yield "one byte", b"x"
    yield "fcheck", bytes([z[0], z[1] ^ 1]) + z[2:]
    flg = 0x20 | ((31 - (0x78 * 256 + 0x20) % 31) % 31)
    yield "fdict", bytes([0x78, flg]) + b"\0\0\0\1" + z[2:]
    yield "btype3", b"\x78\x9c" + bytes([0x07]) + b"\0" * 16
    yield "adler", z[:-1] + bytes([z[-1] ^ 1])
    for i in (3, 100, len(z) // 2, len(z) - 5, len(z) - 1):
        yield f"truncated{i}", z[:i]
    rnd = np.random.default_rng(5)
    for p in rnd.integers(16, len(z) * 8 - 40, 6):
        b = bytearray(z)
        b[p >> 3] ^= 1 << (int(p) & 7)
        yield f"flip{p}", bytes(b)


def test_malformed_on_device(rh):
    """each case once; the host run gives the expected status first, then the device must give the same"""
    for name, b in _malformed():
        want = zlib.decompress(b) if _accepts(b) else None
        hst = _host(b, 1 << 20)
        assert (hst[0] == OK) == (want is not None), name
        assert _device(rh, b, 1 << 20) == hst, name


def _accepts(b):
    try:
        zlib.decompress(b)
        return True
    except zlib.error:
        return False


def test_capacity_and_retry(rh):
    from roibasedimagecompression_amd import RhccqError
    data = _payload(500_000, 6)
    z = zlib.compress(data, 9)
    assert _device(rh, z, 1000) == (CAPACITY, len(data))
    small = zlib.compress(bytes(2_000_000), 9)                 # decodes to far more than the first cap derived from n
    assert rh.to_host(rh.zlib_decompress(small)).tobytes() == bytes(2_000_000)
    with pytest.raises(RhccqError, match="exceeds out_cap"):
        rh.zlib_decompress(z, out_cap=10)
    with pytest.raises(RhccqError, match="incorrect data check"):
        rh.zlib_decompress(z[:-1] + bytes([z[-1] ^ 1]))


def _rhccq_files():
    return sorted(glob.glob(os.path.join(G, "*.rhccq")))


def test_reference_files(rh):
    from roibasedimagecompression_amd.api.uncompression import decompress_color_quantization, load_compressed
    from roibasedimagecompression_amd.container import load_compressed_device, read_frame
    files = _rhccq_files()
    assert len(files) >= 36 and any(f.endswith("g7_lenna64.rhccq") for f in files)
    for f in files:
        host_pkg = load_compressed(f)
        assert load_compressed_device(f, rh) == host_pkg, f
        mirror = decompress_color_quantization(host_pkg)["image"]
        got = read_frame(f, rh)
        assert got["image"].shape == mirror.shape, f
        assert np.array_equal(got["image"].cpu().numpy(), mirror), f
        assert got["shape"] == tuple(host_pkg["s"]) and got["dtype"] == host_pkg.get("d", "uint16"), f


def _frame(rh):
    from roibasedimagecompression_amd import synth
    from roibasedimagecompression_amd.frame import ClassSpec, FrameEncoder
    H, W = 2160, 3840
    img = synth.photo(H, W, 1234)
    (lr, nr, br), (ln, nn, bn) = synth.frame_classes(H, W, (2, 1))
    specs = [ClassSpec(torch.from_numpy(lr).to(rh.device), np.zeros(nr, np.int64), [br], 20),
             ClassSpec(torch.from_numpy(ln).to(rh.device), np.zeros(nn, np.int64), [bn], 20)]
    return FrameEncoder(rh).encode_native(torch.from_numpy(img).to(rh.device), specs)


def test_round_trip_4k_frame(rh, tmp_path):
    from roibasedimagecompression_amd.api.compression import lossless_compress_optimized, save_compressed
    from roibasedimagecompression_amd.container import read_frame, write_frame
    res = _frame(rh)
    pal = torch.from_numpy(np.asarray(res["palette"], np.uint8).reshape(-1, 3)).to(rh.device)
    want = rh.decode(res["indices"].reshape(-1), pal).reshape(res["shape"][0], res["shape"][1], 3)
    fn = str(tmp_path / "dev.rhccq")
    write_frame(res, fn, rh)
    got = read_frame(fn, rh)
    assert torch.equal(got["image"], want)
    assert torch.equal(got["indices"], res["indices"].reshape(-1)) and got["dtype"] == "uint16"
    idx = res["indices"].cpu().numpy().view(np.uint16).reshape(-1)
    fh = str(tmp_path / "host.rhccq")
    save_compressed(lossless_compress_optimized(res["palette"], idx, res["shape"]), fh)   # host zlib level 9
    assert torch.equal(read_frame(fh, rh)["image"], want)


def test_deterministic_with_junk_workspace(rh):
    z = zlib.compress(_payload(700_000, 7), 9)
    want = zlib.decompress(z)
    cap = len(want) + 1000
    ws = rh.zlib_inflate_sizes(len(z), cap)
    outs = []
    for fill in (0x00, 0xFF, 0xA5):
        work = torch.full((ws,), fill, dtype=torch.uint8, device=rh.device)
        out = torch.full((cap,), fill ^ 0x5A, dtype=torch.uint8, device=rh.device)
        o, length, status = rh.zlib_decompress_async(z, cap, out=out, workspace=work)
        ln, st = (int(v[0]) for v in rh.to_host(length, status))
        assert st == OK and ln == len(want)
        outs.append(rh.to_host(o[:ln]).tobytes())
    assert outs[0] == outs[1] == outs[2] == want


def test_queued_calls(rh):
    from roibasedimagecompression_amd.api.uncompression import load_compressed
    pkg = load_compressed(os.path.join(G, "Lenna_compressed_20_10.rhccq"))
    want_p, want_i = zlib.decompress(pkg["p"]), zlib.decompress(pkg["i"])
    p = rh.zlib_decompress_async(pkg["p"], len(want_p) + 5)
    i = rh.zlib_decompress_async(pkg["i"], len(want_i) + 5)     # queued behind the first, no sync between them
    (lp, sp, li, si) = (int(v[0]) for v in rh.to_host(p[1], p[2], i[1], i[2]))
    assert sp == OK and si == OK
    assert rh.to_host(p[0][:lp]).tobytes() == want_p and rh.to_host(i[0][:li]).tobytes() == want_i


def test_abi_argument_errors(rh):
    from roibasedimagecompression_amd import RhccqError
    z = zlib.compress(b"abc" * 1000)
    src = torch.from_numpy(np.frombuffer(z, np.uint8).copy()).to(rh.device)
    ws = rh.zlib_inflate_sizes(len(z), 4096)
    work = torch.empty((ws,), dtype=torch.uint8, device=rh.device)
    out = torch.empty((4096,), dtype=torch.uint8, device=rh.device)
    ln = torch.empty((1,), dtype=torch.int64, device=rh.device)
    st = torch.empty((1,), dtype=torch.int32, device=rh.device)
    P = rh._p
    f = rh.lib.rhccq_zlib_decompress
    assert f(rh.ctx, P(src), -1, P(work), P(out), 4096, P(ln), P(st)) == RHCCQ_E_ARG
    assert f(rh.ctx, None, len(z), P(work), P(out), 4096, P(ln), P(st)) == RHCCQ_E_ARG
    assert f(rh.ctx, P(src), len(z), None, P(out), 4096, P(ln), P(st)) == RHCCQ_E_ARG
    assert f(rh.ctx, P(src), len(z), P(work), None, 4096, P(ln), P(st)) == RHCCQ_E_ARG
    assert f(rh.ctx, P(src), len(z), P(work), P(out), 4096, None, P(st)) == RHCCQ_E_ARG
    assert f(rh.ctx, P(src), len(z), P(work), P(out), 4096, P(ln), None) == RHCCQ_E_ARG
    assert f(rh.ctx, P(src), len(z), P(work), P(out), -1, P(ln), P(st)) == RHCCQ_E_ARG
    assert f(rh.ctx, P(src), len(z), P(work), P(out), 1 << 31, P(ln), P(st)) == RHCCQ_E_LIMIT
    with pytest.raises(RhccqError, match="workspace"):
        rh.zlib_decompress_async(src, 4096, workspace=work[: ws - 1])
    assert f(rh.ctx, P(src), len(z), P(work), P(out), 4096, P(ln), P(st)) == 0
    assert int(st.item()) == OK and rh.to_host(out[: int(ln.item())]).tobytes() == b"abc" * 1000
