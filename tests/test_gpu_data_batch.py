"""GPU: the training data path -- glf_frame_label_sums, glf_prepare_batch, VolumeStore, BatchLoader, ClipLoader and the Trainer
on patient volumes -- bit for bit against the per-sample kernel (data.prepare_frames), oracle.prepare_clip, torch CPU sums
and the window rule of datasets/loader.py:1008-1019 restated on the host."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from oracle import glfusion_ref as orc   # the checker (tests only)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _volume(h0, w0, t, seed):
    """(grey levels 0..255, class ids 0..4) as float32 host volumes [H0, W0, T]; ids beyond a view's parts are dropped."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(h0, w0, t, generator=g) * 256).floor().clamp_(max=255), (torch.rand(h0, w0, t, generator=g) * 5).floor()


# ---------------------------------------------------------------------------------------------------------------- frame sums
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
@pytest.mark.parametrize("h0,w0,t", [(97, 131, 1), (50, 60, 3), (200, 160, 7), (33, 65, 172), (9, 11, 300)])
def test_frame_label_sums_equal_torch(h0, w0, t, dtype):
    """sums[t] = lab.sum(dim=(0, 1)) in int64, exactly; (9, 11, 300) is past the 256 frames one tile of the kernel holds.  The
    output buffer arrives full of garbage: the call writes all of it."""
    from glfusion_amd import data
    from glfusion_amd._lib import check, lib
    g = torch.Generator().manual_seed(h0 + t)
    lab = torch.randint(0, 256 if dtype == torch.uint8 else 5, (h0, w0, t), generator=g).to(dtype)
    want = lab.long().sum(dim=(0, 1))
    dev = lab.to(DEV)
    assert torch.equal(data.frame_label_sums(dev).cpu(), want)
    sums = torch.full((t + 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    check(lib.glf_frame_label_sums(C.c_void_p(dev.data_ptr()), 1 if dtype == torch.uint8 else 0, h0, w0, t,
                                   C.c_void_p(sums.data_ptr() + 8), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert torch.equal(sums[1:-1].cpu(), want) and sums[0].item() == sums[-1].item() == 0x5A5A5A5A5A5A5A5A      # and nothing beyond it


# ------------------------------------------------------------------------------------------------------------ prepare_batch
@pytest.fixture(scope="module")
def volumes():
    """name -> (image, label) host float32 volumes: down-sampling, up-sampling, both, and the identity's 112 x 112."""
    shapes = {"a": (200, 160, 7), "b": (97, 131, 5), "c": (50, 60, 3), "d": (600, 800, 4), "i": (112, 112, 3)}
    return {k: _volume(*s, seed=11 + n) for n, (k, s) in enumerate(shapes.items())}


def _resident(volumes, name, img_u8, lab_u8):
    img, lab = volumes[name]
    return (img.to(torch.uint8) if img_u8 else img).to(DEV), (lab.to(torch.uint8) if lab_u8 else lab).to(DEV)


def _check_batch(volumes, specs):
    """specs: (volume name or None, img uint8?, lab uint8?, t0, nt, view, offset, identity?) per source.  ONE prepare_batch call;
    every source's slice against data.prepare_frames on that source alone and against oracle.prepare_clip."""
    from glfusion_amd import data
    sources, held = [], {}
    for name, iu8, lu8, t0, nt, view, off, ident in specs:
        if name is None:
            sources.append(data.FrameSource(None, None, 0, nt, view))
            continue
        if (name, iu8, lu8) not in held:
            held[name, iu8, lu8] = _resident(volumes, name, iu8, lu8)
        img, lab = held[name, iu8, lu8]
        sources.append(data.FrameSource(img, lab, t0, nt, view, off, 112, 1.0) if ident else data.FrameSource(img, lab, t0, nt, view, off))
    frames, masks = data.prepare_batch(sources, device=DEV)
    total = sum(s[4] for s in specs)
    assert tuple(frames.shape) == (total, 1, 112, 112) and tuple(masks.shape) == (total, 5, 112, 112)
    frames, masks, at = frames.cpu(), masks.cpu(), 0
    for name, iu8, lu8, t0, nt, view, off, ident in specs:
        got_f, got_m = frames[at:at + nt], masks[at:at + nt]
        at += nt
        if name is None:
            assert not got_f.any() and not got_m.any()
            continue
        img, lab = (v[:, :, t0:t0 + nt].contiguous() for v in volumes[name])
        if ident:                  # resize == H0 == W0 == out: the volume's own pixels, frames first; masks = one-hot of the table
            assert torch.equal(got_f, img.permute(2, 0, 1).unsqueeze(1))
            want_m = torch.zeros(nt, 5, 112, 112)
            for cls, ch in enumerate(data.CLASS_TO_CHANNEL[view], start=1):
                if ch >= 0:
                    want_m[:, ch] = (lab.permute(2, 0, 1) == cls).float()
            assert torch.equal(got_m, want_m)
            continue
        one_f, one_m = data.prepare_frames(img.to(DEV), lab.to(DEV), view, crop_offset=off)
        assert torch.equal(got_f, one_f.cpu()) and torch.equal(got_m, one_m.cpu()), (name, t0, nt, view, off)
        ref_f, ref_m = orc.prepare_clip(img, lab, view, off)
        assert torch.equal(got_f, ref_f) and torch.equal(got_m, ref_m), (name, t0, nt, view, off)


def test_prepare_batch_mixed_sources_in_one_call(volumes):
    _check_batch(volumes, [
        ("a", False, False, 0, 1, "4", (0, 0), False),         # float32 / float32, down-sampling, the first frame
        ("b", True, True, 2, 1, "1", (32, 32), False),         # uint8 / uint8, up-sampling, a middle frame
        ("c", True, False, 2, 1, "2", (5, 31), False),         # uint8 image, float32 labels, up-sampling, frame T - 1
        (None, False, False, 0, 2, "3", (0, 0), False),        # a patient without the view: two frames of zeros
        ("d", False, True, 1, 3, "3", (16, 16), False),        # float32 image, uint8 labels, a clip window
        ("i", True, True, 0, 3, "4", (0, 0), True),            # the identity geometry
        ("a", True, True, 6, 1, "1", (5, 31), False),          # the first volume again, as bytes, its last frame
    ])


def test_prepare_batch_one_source(volumes):
    _check_batch(volumes, [("b", True, False, 4, 1, "4", (5, 31), False)])


def test_prepare_batch_more_sources_than_a_chunk(volumes):
    """70 single-frame sources: three launches of at most 32 descriptors, each frame landing in its own place."""
    names, views, offs = ["a", "b", "c", "d"], ["1", "2", "3", "4"], [(0, 0), (32, 32), (5, 31), (16, 16), (31, 0)]
    specs = []
    for k in range(70):
        name = names[k % 4]
        t = volumes[name][0].shape[-1]
        specs.append((None, False, False, 0, 1, "1", (0, 0), False) if k in (31, 64) else
                     (name, k % 3 == 0, k % 2 == 0, (k * 5) % t, 1, views[(k // 4) % 4], offs[k % 5], False))
    _check_batch(volumes, specs)


def test_prepare_batch_image_only_and_errors(volumes):
    from glfusion_amd import data
    img, lab = _resident(volumes, "c", True, True)
    frames, none = data.prepare_batch([data.FrameSource(img, None, 1, 2, "2", (5, 31))], masks=False)
    assert none is None and torch.equal(frames.cpu(), orc.prepare_clip(volumes["c"][0][:, :, 1:3], volumes["c"][1][:, :, 1:3], "2", (5, 31))[0])
    frames, masks = data.prepare_batch([data.FrameSource(img, None, 1, 1, "2")])               # no labels in a batch with masks: zeros
    assert not masks.any() and frames.any()
    with pytest.raises(RuntimeError, match="leave the 3 of the volume"):
        data.prepare_batch([data.FrameSource(img, lab, 2, 2, "2")])
    with pytest.raises(RuntimeError, match="crop window"):
        data.prepare_batch([data.FrameSource(img, lab, 0, 1, "2", (33, 0))])
    with pytest.raises(KeyError):
        data.prepare_batch([data.FrameSource(img, lab, 0, 1, "9")])


# ------------------------------------------------------------------------------------------------------- loader against dataset
VIEWS = ["1", "4"]


def _infos(n_patients=4, missing=()):
    """150 x 170 x 6 volumes: view 1 as uint8 numpy arrays (stored as bytes), view 4 as callables returning float32 tensors."""
    from glfusion_amd import data
    sp = data.SyntheticPatients(VIEWS, n_patients, 6, h0=150, w0=170, device="cpu", seed=21)
    infos = {}
    for k in range(n_patients):
        i1, l1 = sp.volume(k, "1")
        images = {"1": i1.numpy().astype(np.uint8), "4": (lambda k=k: sp.volume(k, "4")[0])}
        labels = {"1": l1.numpy().astype(np.uint8), "4": (lambda k=k: sp.volume(k, "4")[1])}
        for pid, view in missing:
            if pid == k:
                images[view] = None
        infos[f"0_{k}"] = {"dataset_name": "rmyy", "fold": "0", "views_images": images, "views_labels": labels}
    return infos


def _datasets(infos):
    from glfusion_amd import data
    return {v: data.SegPAHDataset(infos, is_train=True, data_list=list(infos), view_num=[v], single_frame=True, device=DEV, crop_seed=5 + int(v))
            for v in VIEWS}


@pytest.fixture(scope="module")
def dataset_batches():
    """What the per-sample path yields in the loader's order -- stacks of ds[i] -- for the complete and the one-view-short infos."""
    from glfusion_amd import data
    out = {}
    for missing in ((), ((2, "4"),)):
        random.seed(17)
        sets = _datasets(_infos(missing=missing))
        plan = data.BatchLoader(sets, 3, store=None).index_plan()
        assert plan == [[3 * k, 3 * k + 1, 3 * k + 2] for k in range(5)]                        # 16 samples: the 16th is dropped
        batches = []
        for idxs in plan:
            items = {v: [sets[v][i] for i in idxs] for v in VIEWS}
            batches.append(({v: torch.stack([it[0] for it in items[v]]).cpu() for v in VIEWS},
                            {v: torch.stack([it[1] for it in items[v]]).cpu() for v in VIEWS}, {v: [it[2] for it in items[v]] for v in VIEWS}))
        out[missing] = batches
    return out


@pytest.mark.parametrize("max_bytes", [1 << 30, 200_000])
@pytest.mark.parametrize("missing", [(), ((2, "4"),)])
def test_batch_loader_equals_the_dataset(dataset_batches, missing, max_bytes):
    """Equal seeds, equal draws: every batch of the loader is the stack of ds[i].  200 000 bytes hold one uint8 volume (153 000)
    and no float32 one (612 000): those are served and dropped, the results do not change, the store stays within its budget."""
    from glfusion_amd import data
    store = data.VolumeStore(DEV, max_bytes)
    random.seed(17)
    loader = data.BatchLoader(_datasets(_infos(missing=missing)), 3, store)
    assert len(loader) == 5
    seen = 0
    for (imgs, masks), (want_i, want_m, want_idx) in zip(loader, dataset_batches[missing]):
        for v in VIEWS:
            assert tuple(imgs[v].shape) == (3, 1, 112, 112) and tuple(masks[v].shape) == (3, 5, 112, 112)
            assert torch.equal(imgs[v].cpu(), want_i[v]) and torch.equal(masks[v].cpu(), want_m[v]) and loader.indices[v] == want_idx[v]
        assert 0 <= store.bytes <= max_bytes and store.bytes == sum(t.numel() * t.element_size() for t in store._volumes.values())
        if max_bytes < (1 << 30):
            assert len(store) <= 1
        seen += 1
    assert seen == 5
    if missing:                                                                                 # patient 2 = samples 8..11 = rows of iterations 2, 3
        rows = [(2, 2), (3, 0), (3, 1), (3, 2)]
        for it, row in rows:
            assert not dataset_batches[missing][it][0]["4"][row].any() and not dataset_batches[missing][it][1]["4"][row].any()
            assert dataset_batches[missing][it][0]["1"][row].any()
    if max_bytes == 1 << 30:
        assert store.loads == 16 - 2 * len(missing)                                            # every volume uploaded once
        assert {t.dtype for k, t in store._volumes.items() if k[1] == "1"} == {torch.uint8}
        assert {t.dtype for k, t in store._volumes.items() if k[1] == "4"} == {torch.float32}


def test_plan_draws_what_getitem_draws():
    """Clip mode too: plan(i) and ds[i] leave `random` and the crop RandomState in the same state, and agree on frames and index."""
    from glfusion_amd import data
    infos = _infos(2)
    store = data.VolumeStore(DEV, 1 << 30)
    for kw in (dict(is_train=True, single_frame=True), dict(is_train=False, single_frame=False, clip_length=5), dict(is_train=True, single_frame=False, clip_length=4)):
        a = data.SegPAHDataset(infos, data_list=list(infos), view_num=["4"], device=DEV, crop_seed=3, **kw)
        b = data.SegPAHDataset(infos, data_list=list(infos), view_num=["4"], device=DEV, crop_seed=3, store=store, **kw)
        for i in range(len(a)):
            random.seed(100 + i)
            img, mask, idx = a[i]
            state = random.getstate()
            random.seed(100 + i)
            plan = b.plan(i)
            assert random.getstate() == state and plan.index == idx
            assert a.R.randint(1 << 30) == b.R.randint(1 << 30)
            frames, masks = data.prepare_batch(plan.sources())
            if kw["single_frame"]:
                assert torch.equal(frames[0], img) and torch.equal(masks[0], mask)
            else:
                assert torch.equal(frames.permute(1, 2, 3, 0), img) and torch.equal(masks.permute(1, 2, 3, 0), mask)


# ------------------------------------------------------------------------------------------------------------------ ClipLoader
def test_clip_loader_follows_the_window_rule():
    from glfusion_amd import data
    rs = np.random.RandomState(4)
    vols = {"0_0": rs.randint(0, 256, size=(112, 112, 3)).astype(np.uint8),                     # fewer frames than clip_length: twice
            "0_1": rs.randint(0, 256, size=(112, 112, 8, 1)).astype(np.float32),                # equal, a trailing singleton axis
            "0_2": rs.randint(0, 256, size=(112, 112, 12)).astype(np.uint8)}                    # more: the first 8
    infos = {k: {"dataset_name": "rmyy", "fold": "0", "views_images": {"4": v}, "views_labels": {"4": np.zeros(v.shape, np.uint8)}}
             for k, v in vols.items()}
    infos["0_3"] = {"dataset_name": "rmyy", "fold": "0", "views_images": {}, "views_labels": {}}   # no view 4: another patient is drawn
    store = data.VolumeStore(DEV, 1 << 30)
    ds = data.AlignedVideoSegPAHDataset(infos, data_list=list(infos), view_num=["4"], clip_length=8)
    loader = data.ClipLoader({"4": ds}, store)
    assert len(loader) == 4
    random.seed(8)
    clips = [c["4"].cpu() for c in loader]
    random.seed(8)
    drawn = "0_3"
    while drawn == "0_3":
        drawn = random.choice(list(infos))
    for clip, pid, frames in zip(clips, ["0_0", "0_1", "0_2", drawn], [6, 8, 8, None]):
        vol = torch.from_numpy(vols[pid].reshape(112, 112, -1)).float()
        t = vol.shape[-1]
        want = torch.cat([vol, vol], dim=2) if t < 8 else vol[:, :, :8]
        assert tuple(clip.shape) == (frames or want.shape[-1], 1, 112, 112) and torch.equal(clip, want.permute(2, 0, 1).unsqueeze(1))
    random.seed(8)
    again = [loader.batch() for _ in range(5)]                                                  # the engine's way in; starts over after the last
    assert all(b[1] is None for b in again) and all(torch.equal(b[0]["4"].cpu(), c) for b, c in zip(again, clips))
    assert torch.equal(again[4][0]["4"].cpu(), clips[0]) and store.loads == 3
    halves = [data.ClipLoader({"4": ds}, store, rank=r, world=2) for r in range(2)]
    random.seed(8)
    assert [len(h) for h in halves] == [2, 2] and torch.equal(next(iter(halves[1]))["4"].cpu(), clips[1])
    wide = {"9_9": dict(infos["0_0"], views_images={"4": np.zeros((112, 96, 8), np.uint8)}, views_labels={"4": np.zeros((112, 96, 8), np.uint8)})}
    with pytest.raises(ValueError, match="square"):
        next(iter(data.ClipLoader({"4": data.AlignedVideoSegPAHDataset(wide, data_list=["9_9"], view_num=["4"], clip_length=8)}, store)))


# --------------------------------------------------------------------------------------------------------------------- Trainer
def _config(tmp_path, **train):
    return {"train": dict({"view_num": ["4"], "test_view": ["4"], "num_epochs": 1, "batch_size": 2, "iters_per_epoch": 1, "clip_length": 24,
                           "save_dir": str(tmp_path), "validate_every_epoch": False, "global_rank": 0}, **train),
            "net": {"opt": {"opt_name": "Adam", "lr": 3e-4, "weight_decay": 1e-5}}}


def test_trainer_trains_from_patient_volumes(tmp_path):
    """infos + video_infos: one epoch of train(is_cycle=True) takes len(loader) steps on BatchLoader batches and ClipLoader clips,
    ends with a finite loss and moved parameters.  The clips are served unresized, so the video volumes are 112 x 112."""
    from glfusion_amd import data
    from glfusion_amd.engine import SyntheticClips, Trainer
    infos = data.synthetic_infos(["4"], 2, clip_length=6, seed=31)
    video = data.synthetic_infos(["4"], 2, clip_length=24, seed=32, h0=112, w0=112)       # seg_cycle: 16 target frames + 8
    random.seed(5)
    np.random.seed(5)
    t = Trainer(_config(tmp_path, infos=infos, video_infos=video, train_list=list(infos), store_bytes=64 << 20))
    assert isinstance(t.loader, data.BatchLoader) and isinstance(t.video_loader, data.ClipLoader)
    assert len(t.loader) == 4 and len(t.video_loader) == 2
    before = [p.detach().clone() for p in t.model.parameters()]
    steps, step = [], t.train_step

    def counted(imgs, masks, video=None):
        assert tuple(imgs["4"].shape) == (2, 1, 112, 112) and tuple(masks["4"].shape) == (2, 5, 112, 112)
        assert tuple(video["4"].shape) == (24, 1, 112, 112) and float(video["4"].max()) > 1.0   # raw grey levels
        steps.append(step(imgs, masks, video))
        return steps[-1]

    t.train_step = counted
    t.train(is_cycle=True)
    assert len(steps) == len(t.loader) == 4
    assert all(bool(torch.isfinite(loss)) for loss, _ in steps)
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, t.model.parameters()))
    assert 0 < t.store.bytes <= 64 << 20
    # without the keys: the synthetic loaders, as before
    plain = Trainer(_config(tmp_path))
    assert isinstance(plain.loader, SyntheticClips) and isinstance(plain.video_loader, SyntheticClips)
    # real batches beside noise clips: refused
    half = Trainer(_config(tmp_path, infos=infos, train_list=list(infos)))
    assert isinstance(half.loader, data.BatchLoader) and isinstance(half.video_loader, SyntheticClips)
    with pytest.raises(ValueError, match="video_infos"):
        half.train(is_cycle=True)
