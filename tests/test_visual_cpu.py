"""CPU: the visual mode's C entry points (glf_render_labels, glf_restore_labels) are declared, exported and refuse bad arguments
before they touch the HIP runtime; the restatement in tests/visual_ref.py equals the reference's literal formula (main.py:606-612);
the palette and class tables; the PNG writer; no CPU fallback."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import visual_ref as V
from glfusion_amd import _lib, data, png
from glfusion_amd._lib import lib

GLF_ERR_BAD_SHAPE, GLF_ERR_NULL = -1, -5
P, I = C.c_void_p, C.c_int
SIGNATURES = {
    "glf_render_labels": [P, P, P, P, I, I, I, I, P, I, P],
    "glf_restore_labels": [P, P, I, I, I, I, I, I, I, I, I, P, P],
}


def _err():
    return lib.glf_last_error()


def test_header_declares_and_library_exports_the_visual_functions():
    protos = _lib.parse_header()
    dll = C.CDLL(_lib.LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        assert name in protos, name
        assert protos[name][0] is C.c_int and protos[name][1] == argtypes, name
        assert hasattr(dll, name), name
    dll.glf_abi_version.restype = C.c_int
    assert dll.glf_abi_version() == 7                      # additive: the ABI version does not move
    text = open(_lib.HEADER).read()
    assert all(text.index("int glf_overlap_counts_nchw(") < text.index(f"int {name}(") for name in SIGNATURES)
    # declared after glf_overlap_counts_nchw behind a comment block of their own
    assert re.search(r"glf_overlap_counts_nchw\s*\([^;]*\);\s*/\*.*?\*/\s*int glf_render_labels\s*\(", text, flags=re.S)


def _host_buffers():
    # stand-ins for the device arrays: checked for null / alignment only, never read or written by the host
    buf = (C.c_int64 * 8)()
    base = C.addressof(buf)
    assert base % 8 == 0
    return buf, base


def test_render_labels_argument_checks_need_no_gpu():
    keep, dev = _host_buffers()
    pal = (C.c_uint8 * 24)(*[x for row in data.PALETTE for x in row])

    def call(logits=dev, frames=None, labels=dev + 16, rgba=dev + 32, n=1, c=5, h=1, w=1, palette=pal, alpha=255):
        return lib.glf_render_labels(logits, frames, labels, rgba, n, c, h, w, palette, alpha, None)

    assert call(logits=None) == GLF_ERR_NULL and b"render_labels: null logits" in _err()
    assert call(labels=None, rgba=None) == GLF_ERR_NULL and b"render_labels" in _err() and b"both null" in _err()
    assert call(palette=None) == GLF_ERR_NULL and b"render_labels: null palette" in _err()
    # a null pointer wins over every other error
    assert call(logits=None, n=0, c=9, alpha=-1, rgba=dev + 33) == GLF_ERR_NULL
    assert call(palette=None, n=0, alpha=300) == GLF_ERR_NULL
    for bad in (dict(n=0), dict(c=0), dict(h=0), dict(w=0), dict(n=-3), dict(w=-1)):
        assert call(**bad) == GLF_ERR_BAD_SHAPE and b"render_labels" in _err() and b"must be > 0" in _err(), bad
    assert call(c=9) == GLF_ERR_BAD_SHAPE and b"render_labels" in _err() and b"at most 8" in _err()
    for alpha in (-1, 256):
        assert call(alpha=alpha) == GLF_ERR_BAD_SHAPE and b"render_labels: alpha" in _err()
        assert call(alpha=alpha, frames=dev) == GLF_ERR_BAD_SHAPE and b"render_labels: alpha" in _err()
    for off in (1, 2, 3):
        assert call(rgba=dev + 32 + off) == GLF_ERR_BAD_SHAPE and b"render_labels: rgba must be 4-byte aligned" in _err()
    assert call(n=0, rgba=dev + 33) == GLF_ERR_BAD_SHAPE and b"must be > 0" in _err()          # extents before support


def test_restore_labels_argument_checks_need_no_gpu():
    keep, dev = _host_buffers()
    table = (C.c_int * 8)(3, 4, 2, 1, 0, 0, 0, 0)

    def call(logits=dev, volume=dev + 32, t=1, c=5, oh=112, ow=112, h0=10, w0=10, resize=144, oy=16, ox=16, tab=table):
        return lib.glf_restore_labels(logits, volume, t, c, oh, ow, h0, w0, resize, oy, ox, tab, None)

    assert call(logits=None) == GLF_ERR_NULL and b"restore_labels: null logits" in _err()
    assert call(volume=None) == GLF_ERR_NULL and b"restore_labels: null volume" in _err()
    assert call(tab=None) == GLF_ERR_NULL and b"restore_labels: null channel_to_class" in _err()
    assert call(tab=None, t=0, c=9, oy=100) == GLF_ERR_NULL                                   # a null pointer wins over every other error
    for bad in (dict(t=0), dict(c=0), dict(oh=0), dict(ow=0), dict(h0=0), dict(w0=0), dict(resize=0), dict(t=-1)):
        assert call(**bad) == GLF_ERR_BAD_SHAPE and b"restore_labels: sizes must be > 0" in _err(), bad
    assert call(c=9) == GLF_ERR_BAD_SHAPE and b"restore_labels" in _err() and b"at most 8" in _err()
    for value in (-1, 256):
        assert call(tab=(C.c_int * 5)(1, 2, value, 0, 0)) == GLF_ERR_BAD_SHAPE and b"restore_labels: channel_to_class[2]" in _err()
    for bad in (dict(oy=33), dict(ox=33), dict(oy=-1), dict(ox=-1), dict(oh=145, oy=0), dict(resize=100)):
        assert call(**bad) == GLF_ERR_BAD_SHAPE and b"restore_labels" in _err() and b"crop window" in _err(), bad


def _inputs(seed, shape):
    g = torch.Generator().manual_seed(seed)
    return V.plant(torch.randn(*shape, generator=g) * 3)


@pytest.mark.parametrize("shape", [(1, 5, 1, 1), (3, 5, 5, 7), (2, 1, 9, 65), (2, 8, 9, 65), (2, 5, 112, 112)])
def test_restatement_equals_the_reference_formula(shape):
    x = _inputs(shape[2] * 31 + shape[1], shape)
    assert torch.equal(V.labels_ref(x).long(), V.literal_labels(x))
    masks = (torch.rand(*shape, generator=torch.Generator().manual_seed(3)) < 0.3).float()      # several channels set: not one-hot
    assert torch.equal(V.labels_ref(masks).long(), V.literal_labels(masks))
    if shape[1] == 5 and shape[2] > 1:
        assert set(V.labels_ref(x).unique().tolist()) == {0, 1, 2, 3, 4, 5}


def test_restatement_on_planted_values():
    for value, on in [(0.0, False), (-0.0, False), (1e-3, True), (-1e-3, False), (float("inf"), True), (float("-inf"), False)]:
        x = torch.full((1, 5, 2, 3), -4.0)
        x[0, 3, 1, 2] = value
        x[0, 4, 1, 2] = 1.0                                                  # a higher channel that is on: masked by channel 3 when it is on
        want = V.literal_labels(x)
        assert int(want[0, 1, 2]) == (4 if on else 5) and int(want.sum()) == int(want[0, 1, 2]), value
        assert torch.equal(V.labels_ref(x).long(), want), value
    x = torch.full((1, 5, 1, 1), float("nan"))                              # NaN > 0.5 is false: off
    assert int(V.labels_ref(x)) == 0 and int(V.literal_labels(x)) == 0


def test_restore_restatement_tie_break_window_and_tables():
    x = torch.full((1, 5, 112, 112), -5.0)
    x[0, 1, 0, 0] = x[0, 3, 0, 0] = 2.0                                     # a tie: the lower channel's class
    x[0, 1, 0, 1], x[0, 3, 0, 1] = 2.0, 3.0                                  # the larger logit's class
    x[0, 4, 0, 2] = 9.0                                                      # view 1 does not show channel 4
    x[0, 4, 0, 3], x[0, 3, 0, 3] = 9.0, 0.5                                  # ... and it does not outvote a shown channel either
    vol = V.restore_ref(x, data.CHANNEL_TO_CLASS["1"], (144, 144))
    assert tuple(vol.shape) == (144, 144, 1) and vol.dtype == torch.uint8
    assert vol[16, 16:20, 0].tolist() == [2, 1, 0, 1] and int(vol.sum()) == 4
    win = V.window_ref((144, 144))
    assert int(win.sum()) == 112 * 112 and bool(win[16:128, 16:128].all())
    win = V.window_ref((150, 170))
    assert not win[0].any() and not win[:, 0].any() and not win[-1].any() and not win[:, -1].any() and 0 < int(win.sum()) < 150 * 170


def test_palette_is_the_references():
    assert [list(row) for row in data.PALETTE] == [[0, 0, 0, 255], [55, 255, 254, 255], [27, 255, 46, 255], [45, 0, 251, 255],
                                                   [251, 13, 15, 255], [223, 48, 236, 255]]


def test_channel_to_class_inverts_class_to_channel():
    assert set(data.CHANNEL_TO_CLASS) == set(data.CLASS_TO_CHANNEL)
    for v, table in data.CLASS_TO_CHANNEL.items():
        inv = data.CHANNEL_TO_CLASS[v]
        assert len(inv) == 5
        shown = {ch: k + 1 for k, ch in enumerate(table) if ch >= 0}
        for k, ch in enumerate(table):
            if ch >= 0:
                assert inv[ch] == k + 1
        assert all(inv[ch] == shown.get(ch, 0) for ch in range(5))


def _pillow():
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (112, 112)])
def test_png_round_trip(tmp_path, h, w):
    a = np.random.RandomState(h * 131 + w).randint(0, 256, size=(h, w, 4)).astype(np.uint8)
    path = tmp_path / "a.png"
    png.write_rgba(path, a)
    assert np.array_equal(V.decode_png(path), a)
    Image = _pillow()
    if Image is not None:
        with Image.open(path) as im:
            assert im.mode == "RGBA" and im.size == (w, h) and np.array_equal(np.asarray(im), a)
    png.write_rgba(str(path), np.ascontiguousarray(a[::-1]))               # a str path too; overwrites
    assert np.array_equal(V.decode_png(path), a[::-1])


def test_png_refuses_other_dtypes_and_shapes(tmp_path):
    for bad in (np.zeros((4, 4, 4), np.float32), np.zeros((4, 4, 4), np.float64), np.zeros((4, 4, 3), np.uint8),
                np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.int8), np.zeros((0, 4, 4), np.uint8), [[[0, 0, 0, 255]]]):
        with pytest.raises(ValueError, match="uint8"):
            png.write_rgba(tmp_path / "bad.png", bad)
    assert not (tmp_path / "bad.png").exists()


def test_render_and_restore_have_no_cpu_fallback():
    x = torch.zeros(2, 5, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        data.render_labels(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        data.render_labels(x, frames=torch.zeros(2, 1, 4, 4), alpha=96)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        data.restore_labels(torch.zeros(2, 5, 112, 112), "4", (150, 170))
    with pytest.raises(KeyError):
        data.restore_labels(torch.zeros(2, 5, 112, 112), "9", (150, 170))
