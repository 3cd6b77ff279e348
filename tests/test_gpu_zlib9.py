"""The exact level-9 zlib encoder on the device (csrc/zlib_deflate9.hip, rhccq_zlib9_compress): the device stream equals
the host twin and the golden layers, live zlib.compress(x, 9) where the installed zlib reproduces the golden layers, does
not depend on the workspace or the stream, and write_frame(exact=True) writes the host path's file byte for byte."""
import ctypes as C
import glob
import hashlib
import json
import logging
import os
import pickle
import struct
import time
import zlib

import numpy as np
import pytest
import torch

from test_zlib9_cpu import LIVE, _LAYERS, _SYN, z9

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
RHCCQ_E_ARG, RHCCQ_E_LIMIT = -1, -3
log = logging.getLogger(__name__)


@pytest.fixture(scope="module")
def rh():
    from roibasedimagecompression_amd.ops import Rhccq
    return Rhccq(0)


def _dev(rh, data):
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(rh.device)


def _exact(rh, data):
    return rh.zlib_compress(_dev(rh, data), exact=True)


def test_golden_layers_device(rh):
    for name, raw, want in _LAYERS:
        assert _exact(rh, raw) == want, name


@pytest.mark.parametrize("name", sorted(_SYN))
def test_synthetic_device_equals_host_twin(rh, name):
    x = _SYN[name]
    y = _exact(rh, x)
    assert y == z9(x)
    assert zlib.decompress(y) == x
    if LIVE:
        assert y == zlib.compress(x, 9)


def test_workspace_and_stream_independence(rh):
    x = _SYN["flat_uint16_map_big"] + _SYN["random_run_random"]
    t = _dev(rh, x)
    ws, bound = rh.zlib_sizes(t.numel(), exact=True)
    want = z9(x)
    outs = []
    for fill in (0, 0xFF, 0x5A):
        work = torch.full((ws,), fill, dtype=torch.uint8, device=rh.device)
        out = torch.full((bound,), fill ^ 0x33, dtype=torch.uint8, device=rh.device)
        o, n = rh.zlib_compress_async(t, out=out, workspace=work, exact=True)
        outs.append(bytes(o[: int(n.item())].cpu().numpy()))
    side = torch.cuda.Stream(rh.device)
    with torch.cuda.stream(side):
        outs.append(rh.zlib_compress(t, exact=True))
    side.synchronize()
    assert all(o == want for o in outs)


def test_stats(rh):
    x = _SYN["lowalpha4_200k"]
    t = _dev(rh, x)
    ws, bound = rh.zlib_sizes(t.numel(), exact=True)
    work = torch.empty((ws,), dtype=torch.uint8, device=rh.device)
    out, n = rh.zlib_compress_async(t, workspace=work, exact=True)
    cand, nodes, rounds, stored, fixed, dyn = rh.zlib9_stats(t.numel(), work)
    assert cand > len(x) and 0 < nodes <= len(x) and rounds >= 1
    assert stored + fixed + dyn >= 1
    assert bytes(out[: int(n.item())].cpu().numpy()) == z9(x)


def test_collision_heavy_4mib(rh):
    keys = [bytes([(k << 5) | 3, 9, 17]) for k in range(8)]
    rng = np.random.default_rng(77)
    x = b"".join(keys[i] for i in rng.integers(0, 8, (4 << 20) // 3))
    t = _dev(rh, x)
    rh.zlib_compress(t[:4096], exact=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    y = rh.zlib_compress(t, exact=True)
    ms = 1e3 * (time.perf_counter() - t0)
    log.warning("collision-heavy 4 MiB: %.1f ms, %d -> %d bytes", ms, len(x), len(y))
    assert zlib.decompress(y) == x
    if LIVE:
        assert y == zlib.compress(x, 9)


def test_reference_files_reencoded(rh):
    kat = json.load(open(os.path.join(G, "g8_rhccq_kat.json")))
    known = {v["file_sha256"] for v in kat.values()}
    seen = 0
    for f in sorted(glob.glob(os.path.join(G, "*.rhccq"))):
        raw = open(f, "rb").read()
        if hashlib.sha256(raw).hexdigest() not in known:
            continue
        body = raw[9:9 + struct.unpack("<I", raw[5:9])[0]]
        pkg = pickle.loads(zlib.decompress(body))
        for k in ("p", "i"):
            pkg[k] = _exact(rh, zlib.decompress(pkg[k]))
        outer = _exact(rh, pickle.dumps(pkg, protocol=5))
        rebuilt = b"RHCCQ" + struct.pack("<I", len(outer)) + outer
        assert hashlib.sha256(rebuilt).hexdigest() == hashlib.sha256(raw).hexdigest(), f
        seen += 1
    assert seen >= 30


def test_write_frame_exact_lenna(rh, tmp_path):
    from roibasedimagecompression_amd.api.compression import lossless_compress_optimized, save_compressed
    from roibasedimagecompression_amd.api.uncompression import load_compressed, lossless_decompress
    from roibasedimagecompression_amd.container import write_frame
    pal, idx, shape = lossless_decompress(load_compressed(os.path.join(G, "Lenna_compressed_20_10.rhccq")))
    save_compressed(lossless_compress_optimized(pal, idx, shape), str(tmp_path / "host.rhccq"))
    res = {"palette": pal, "indices": np.asarray(idx), "shape": shape}
    write_frame(res, str(tmp_path / "dev.rhccq"), rh, exact=True)
    assert (tmp_path / "dev.rhccq").read_bytes() == (tmp_path / "host.rhccq").read_bytes()


def test_write_frame_exact_4k_frame(rh, tmp_path):
    from roibasedimagecompression_amd import synth
    from roibasedimagecompression_amd.api.compression import lossless_compress_optimized, save_compressed
    from roibasedimagecompression_amd.container import narrow_indices, write_frame
    from roibasedimagecompression_amd.frame import ClassSpec, FrameEncoder
    H, W = 2160, 3840
    img = synth.photo(H, W, 1234)
    (lr, nr, br), (ln, nn, bn) = synth.frame_classes(H, W, (2, 1))
    specs = [ClassSpec(torch.from_numpy(lr).to(rh.device), np.zeros(nr, np.int64), [br], 20),
             ClassSpec(torch.from_numpy(ln).to(rh.device), np.zeros(nn, np.int64), [bn], 20)]
    res = FrameEncoder(rh).encode_native(torch.from_numpy(img).to(rh.device), specs)
    idx = res["indices"].cpu().numpy().view(np.uint16).reshape(-1)
    save_compressed(lossless_compress_optimized(res["palette"], idx, res["shape"]), str(tmp_path / "host.rhccq"))
    write_frame(res, str(tmp_path / "dev.rhccq"), rh, exact=True)
    assert (tmp_path / "dev.rhccq").read_bytes() == (tmp_path / "host.rhccq").read_bytes()
    raw = bytes(narrow_indices(res["indices"], rh)[0].cpu().numpy())
    y = _exact(rh, raw)
    assert y == z9(raw)
    if LIVE:
        assert y == zlib.compress(raw, 9)


def test_abi_errors(rh):
    from roibasedimagecompression_amd import RhccqError
    lib = rh._raw
    ws, bound = C.c_int64(), C.c_int64()
    assert lib.rhccq_zlib9_sizes(-1, C.byref(ws), C.byref(bound)) == RHCCQ_E_ARG
    assert lib.rhccq_zlib9_sizes(1 << 31, C.byref(ws), C.byref(bound)) == RHCCQ_E_LIMIT
    t = _dev(rh, bytes(range(256)) * 64)
    wsz, bnd = rh.zlib_sizes(t.numel(), exact=True)
    work = torch.empty((wsz,), dtype=torch.uint8, device=rh.device)
    out = torch.empty((bnd,), dtype=torch.uint8, device=rh.device)
    length = torch.empty((1,), dtype=torch.int64, device=rh.device)
    a = (rh._p(work), rh._p(out))
    f = rh.lib.rhccq_zlib9_compress
    assert f(rh.ctx, rh._p(t), -1, *a, bnd, rh._p(length)) == RHCCQ_E_ARG
    assert f(rh.ctx, None, t.numel(), *a, bnd, rh._p(length)) == RHCCQ_E_ARG
    assert f(rh.ctx, rh._p(t), t.numel(), None, rh._p(out), bnd, rh._p(length)) == RHCCQ_E_ARG
    assert f(rh.ctx, rh._p(t), t.numel(), *a, bnd, None) == RHCCQ_E_ARG
    assert f(rh.ctx, rh._p(t), t.numel(), *a, bnd - 1, rh._p(length)) == RHCCQ_E_ARG
    assert f(rh.ctx, rh._p(t), 1 << 31, *a, bnd, rh._p(length)) == RHCCQ_E_LIMIT
    with pytest.raises(RhccqError):
        rh.zlib_compress_async(t, out=out[:bnd - 1], exact=True)
    assert _exact(rh, bytes(range(256)) * 64) == z9(bytes(range(256)) * 64)


def test_default_stays_fast_encoder(rh, monkeypatch):
    t = _dev(rh, _SYN["runs"])
    calls = []
    raw = rh.lib.rhccq_zlib_compress
    monkeypatch.setattr(rh.lib, "rhccq_zlib_compress", lambda *a: calls.append(1) or raw(*a))
    y = rh.zlib_compress(t)
    assert calls == [1]
    assert zlib.decompress(y) == _SYN["runs"]
    monkeypatch.undo()
    assert y == rh.zlib_compress(t)
