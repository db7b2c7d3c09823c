"""CPU: the training data path's C entry points (glf_frame_label_sums, glf_prepare_batch) are declared, exported and refuse bad
arguments before they touch the HIP runtime; BatchLoader's host-only index plan; AlignedVideoSegPAHDataset's window rule
(datasets/loader.py:1008-1019) on host arrays; no CPU fallback."""
import ctypes as C
import random
import re

import numpy as np
import pytest
import torch

from glfusion_amd import _lib, data
from glfusion_amd._lib import FrameSrc, lib

GLF_ERR_BAD_SHAPE, GLF_ERR_UNSUPPORTED, GLF_ERR_NULL = -1, -2, -5
P, I = C.c_void_p, C.c_int
SIGNATURES = {
    "glf_frame_label_sums": [P, I, I, I, I, P, P],
    "glf_prepare_batch": [P, I, P, P, I, I, P],
}


def _err():
    return lib.glf_last_error()


def test_header_declares_and_library_exports_the_batch_functions():
    protos = _lib.parse_header()
    dll = C.CDLL(_lib.LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        assert name in protos, name
        assert protos[name][0] is C.c_int and protos[name][1] == argtypes, name
        assert hasattr(dll, name), name
    dll.glf_abi_version.restype = C.c_int
    assert dll.glf_abi_version() == 7                      # additive: the ABI version does not move
    text = open(_lib.HEADER).read()
    assert all(text.index("int glf_restore_labels(") < text.index(f"int {name}(") for name in SIGNATURES)
    # declared after glf_restore_labels behind a comment block of their own
    assert re.search(r"glf_restore_labels\s*\([^;]*\);\s*/\*.*?\*/", text, flags=re.S)
    assert C.sizeof(FrameSrc) == 80                       # the mirror of glf_frame_src: 2 pointers, 14 int32, 1 float, 1 reserved
    m = re.search(r"typedef struct \{([^}]*)\} glf_frame_src;", text)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", m.group(1)))
    assert names == [f[0] for f in FrameSrc._fields_]


def _host_buffers():
    # stand-ins for the device arrays: checked for null only, never read or written by the host
    buf = (C.c_int64 * 8)()
    return buf, C.addressof(buf)


def test_frame_label_sums_argument_checks_need_no_gpu():
    keep, dev = _host_buffers()

    def call(lab=dev, dtype=1, h0=4, w0=4, t=3, sums=dev + 32):
        return lib.glf_frame_label_sums(lab, dtype, h0, w0, t, sums, None)

    assert call(lab=None) == GLF_ERR_NULL and b"frame_label_sums: null" in _err()
    assert call(sums=None) == GLF_ERR_NULL and b"frame_label_sums: null" in _err()
    assert call(lab=None, t=0, dtype=7) == GLF_ERR_NULL                                   # a null pointer wins over every other error
    for bad in (dict(h0=0), dict(w0=0), dict(t=0), dict(t=-2)):
        assert call(**bad) == GLF_ERR_BAD_SHAPE and b"frame_label_sums" in _err() and b"must be > 0" in _err(), bad
    for dtype in (-1, 2):
        assert call(dtype=dtype) == GLF_ERR_UNSUPPORTED and b"frame_label_sums: dtype" in _err()


def _src(dev, **kw):
    d = FrameSrc()
    d.img, d.lab, d.img_dtype, d.lab_dtype = dev, dev + 16, 1, 0
    d.H0, d.W0, d.T, d.t0, d.nt, d.resize, d.off_y, d.off_x, d.img_div = 50, 60, 6, 2, 1, 144, 5, 31, 255.0
    d.class_to_channel[:] = (3, 2, 0, 1)
    for k, v in kw.items():
        if k == "class_to_channel":
            d.class_to_channel[:] = v
        else:
            setattr(d, k, v)
    return d


def test_prepare_batch_argument_checks_need_no_gpu():
    keep, dev = _host_buffers()

    def call(srcs, n=None, out_img=dev + 32, out_mask=dev + 48, oh=112, ow=112):
        arr = (FrameSrc * len(srcs))(*srcs) if srcs is not None else None
        return lib.glf_prepare_batch(arr, len(srcs) if n is None else n, out_img, out_mask, oh, ow, None)

    assert call(None, n=1) == GLF_ERR_NULL and b"prepare_batch: null source" in _err()
    assert call([_src(dev)], out_img=None) == GLF_ERR_NULL and b"prepare_batch: null out_img" in _err()
    assert call(None, n=0) == GLF_ERR_NULL                                                # a null pointer wins over every other error
    for n in (0, -1):
        assert call([_src(dev)], n=n) == GLF_ERR_BAD_SHAPE and b"prepare_batch: n =" in _err()
    # t0 + nt > T, in the second of two sources: every descriptor is checked, and the message names it
    for bad in (dict(t0=6), dict(t0=5, nt=2), dict(t0=0, nt=7), dict(t0=-1), dict(t0=2**31 - 1, nt=2)):
        assert call([_src(dev), _src(dev, **bad)]) == GLF_ERR_BAD_SHAPE and b"prepare_batch: source 1: frames" in _err(), bad
    assert call([_src(dev, nt=0)]) == GLF_ERR_BAD_SHAPE and b"nt = 0" in _err()
    assert call([_src(dev, img=None, nt=0)]) == GLF_ERR_BAD_SHAPE and b"nt = 0" in _err()       # a zero source still has frames
    for bad in (dict(off_y=33), dict(off_x=33), dict(off_y=-1), dict(off_x=-1), dict(resize=100), dict(resize=112, off_y=1)):
        assert call([_src(dev, **bad)]) == GLF_ERR_BAD_SHAPE and b"prepare_batch: source 0" in _err() and b"crop window" in _err(), bad
    assert call([_src(dev, H0=112, W0=112, resize=112, off_y=0, off_x=0)], oh=113) == GLF_ERR_BAD_SHAPE and b"crop window" in _err()
    for bad in (dict(img_dtype=2), dict(img_dtype=-1), dict(lab_dtype=2), dict(lab_dtype=-1)):
        assert call([_src(dev, **bad)]) == GLF_ERR_UNSUPPORTED and b"prepare_batch: source 0" in _err() and b"dtype" in _err(), bad
    for table in ((3, 2, 0, 5), (-2, 1, 0, 1), (3, 2, 99, 1)):
        assert call([_src(dev, class_to_channel=table)]) == GLF_ERR_BAD_SHAPE and b"channel index out of range" in _err(), table
    for bad in (dict(H0=0), dict(W0=0), dict(T=0), dict(resize=0)):
        assert call([_src(dev, **bad)]) == GLF_ERR_BAD_SHAPE and b"sizes must be > 0" in _err(), bad
    assert call([_src(dev, img_div=0.0)]) == GLF_ERR_BAD_SHAPE and b"img_div" in _err()
    assert call([_src(dev)], oh=0) == GLF_ERR_BAD_SHAPE and b"output extents" in _err()


def test_prepare_batch_and_frame_sums_have_no_cpu_fallback():
    vol = torch.zeros(8, 8, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        data.prepare_batch([data.FrameSource(vol, vol, 0, 1, "4")])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        data.prepare_batch([data.FrameSource(None, None, 0, 1, "4")])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        data.frame_label_sums(vol)
    with pytest.raises(RuntimeError, match="no sources"):
        data.prepare_batch([])


class _Sized:
    view_num, seg_parts = ["4"], True

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


@pytest.mark.parametrize("world", [1, 2])
def test_batch_loader_index_plan(world):
    """11 samples, B = 2: 5 iterations of consecutive indices, the 11th sample dropped; over 2 ranks disjoint stripes of 2."""
    plans = [data.BatchLoader({"4": _Sized(11), "1": _Sized(11)}, 2, store=None, rank=r, world=world).index_plan() for r in range(world)]
    whole = [[2 * k, 2 * k + 1] for k in range(5)]
    if world == 1:
        assert plans[0] == whole
    else:
        assert plans[0] == [whole[0], whole[2]] and plans[1] == [whole[1], whole[3]]            # iteration 4 dropped: equal lengths
    for r, plan in enumerate(plans):
        assert len(plan) == len(data.BatchLoader({"4": _Sized(11)}, 2, store=None, rank=r, world=world)) == 5 // world
        assert all(idxs == list(range(idxs[0], idxs[0] + 2)) for idxs in plan)
    flat = [i for plan in plans for idxs in plan for i in idxs]
    assert len(flat) == len(set(flat)) and max(flat) < 10
    with pytest.raises(ValueError):
        data.BatchLoader({"4": _Sized(11)}, 2, store=None, rank=world, world=world)


def _video_infos(t, trailing=False):
    rs = np.random.RandomState(t)
    infos = {}
    for k in range(3):
        shape = (5, 7, t, 1) if trailing else (5, 7, t)
        img = rs.randint(0, 256, size=shape).astype(np.uint8)
        lab = rs.randint(0, 5, size=shape).astype(np.uint8)
        has = k != 1                                                                             # patient 1 lacks the view
        infos[f"0_{k}"] = {"dataset_name": "rmyy", "fold": "0", "views_images": {"4": img} if has else {"4": None},
                           "views_labels": {"4": lab} if has else {}}
    return infos


@pytest.mark.parametrize("t", [3, 8, 12])
@pytest.mark.parametrize("random_sample", [False, True])
def test_aligned_video_window_rule(t, random_sample):
    """loader.py:1008-1019 at clip_length 8: T = 12 -> 8 frames (the first, or from random.randint(0, T - 8 - 1)); T = 3 -> the
    volume twice; T = 8 -> unchanged.  Raw grey levels [1, H, W, T'], index 0; a patient without the view -> random.choice."""
    infos = _video_infos(t, trailing=(t == 8))
    ids = list(infos)
    ds = data.AlignedVideoSegPAHDataset(infos, is_train=True, data_list=ids, view_num=["4"], clip_length=8, random_sample=random_sample)
    assert len(ds) == 3
    for index in (0, 2, 1):
        random.seed(40 + index)
        images, masks, idx = ds[index]
        random.seed(40 + index)                                                                  # the draws restated, in order
        pid = ids[index]
        while infos[pid]["views_images"].get("4") is None or infos[pid]["views_labels"].get("4") is None:
            pid = random.choice(ids)
        assert pid != "0_1"
        vol, lab = infos[pid]["views_images"]["4"].reshape(5, 7, t), infos[pid]["views_labels"]["4"].reshape(5, 7, t)
        if t > 8:
            start = random.randint(0, t - 8 - 1) if random_sample else 0
            want, want_lab = vol[:, :, start:start + 8], lab[:, :, start:start + 8]
        elif t < 8:
            want, want_lab = np.concatenate([vol, vol], axis=2), np.concatenate([lab, lab], axis=2)
        else:
            want, want_lab = vol, lab
        assert idx == 0 and images.dtype == torch.uint8 and tuple(images.shape) == (1, 5, 7, {3: 6, 8: 8, 12: 8}[t])
        assert torch.equal(images, torch.from_numpy(want).unsqueeze(0))
        assert masks.dtype == torch.float32 and torch.equal(masks, torch.from_numpy(want_lab).float())
    ds_id = data.AlignedVideoSegPAHDataset(infos, data_list=ids, view_num=["4"], clip_length=8, require_id=True)
    random.seed(1)
    assert ds_id[1][3] == "0_1" and ds_id[1][2] == 0                                             # the id asked for, as in the reference
    none = {k: dict(v, views_images={}, views_labels={}) for k, v in infos.items()}
    with pytest.raises(RuntimeError, match="no patient"):
        data.AlignedVideoSegPAHDataset(none, data_list=ids, view_num=["4"], clip_length=8)[0]


def test_aligned_video_id_split_is_the_references():
    infos = {f"0_{k}": {"dataset_name": "rmyy" if k % 5 else "gy", "fold": "0", "views_images": {}, "views_labels": {}} for k in range(20)}
    random.seed(9)
    ds = data.AlignedVideoSegPAHDataset(infos, is_train=True, view_num=["2"])
    random.seed(9)
    ids = [k for k, v in infos.items() if v["dataset_name"] == "rmyy"]
    train = random.sample(ids, int(len(ids) * 0.8))
    assert ds.id_list == train and len(ds) == 12 and set(ds.valid_list) | set(ds.test_list) == set(ids) - set(train)
    random.seed(9)
    assert data.SegPAHDataset(infos, is_train=True, view_num=["2"]).id_list == train           # one split for both datasets
    assert len(data.AlignedVideoSegPAHDataset(infos, is_train=False, view_num=["2"])) == 16


def test_load_infos(tmp_path):
    infos = {"0_0": {"dataset_name": "rmyy", "fold": "0", "views_images": {"4": "a.nii.gz"}, "views_labels": {"4": "b.nii.gz"}}}
    np.save(tmp_path / "infos.npy", infos, allow_pickle=True)
    assert data.load_infos(infos) is infos and data.load_infos(str(tmp_path / "infos.npy")) == infos
    with pytest.raises(TypeError):
        data.load_infos([1, 2])
