"""GPU: glf_contour_distances, data.contour_metrics and the engine's contour report against the numpy restatement
(tests/contour_ref.py).  Integer fields are compared for equality.  sum_d and the derived HD / HDpct / ASSD are compared within 1e-9
relative: at most 12 544 terms (50 176 at 224 x 224), each a correctly rounded square root, added in another order, differ by less
than 50 176 * 2^-53 < 6e-12 relative -- the bound is derived, not measured."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

import contour_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL = 1e-9
ON_LOGITS = np.array([np.inf, 1e-3, 3.0, 0.7, 2e-4], dtype=np.float32)
OFF_LOGITS = np.array([0.0, -0.0, -np.inf, np.nan, -1e-3, -2.0, -2e-4], dtype=np.float32)
ON_TARGETS = np.array([1.0, 1.0, 0.5, -1.0], dtype=np.float32)
OFF_TARGETS = np.array([0.0, -0.0], dtype=np.float32)


def _encode(mask, on_values, off_values, rng):
    on = on_values[rng.integers(0, len(on_values), size=mask.shape)]
    off = off_values[rng.integers(0, len(off_values), size=mask.shape)]
    return np.where(mask, on, off).astype(np.float32)


def _disc(h, w, r):
    yy, xx = np.mgrid[:h, :w]
    return (yy - h // 2) ** 2 + (xx - w // 2) ** 2 <= r * r


def _families(h, w, seed):
    """(name, prediction mask, target mask) of one plane size: every family of the issue."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    empty, full = np.zeros((h, w), bool), np.ones((h, w), bool)
    out = []
    corners = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    for k, (y, x) in enumerate(corners):
        a, b = empty.copy(), empty.copy()
        a[y, x] = True
        b[corners[3 - k]] = True
        out.append((f"corner{k}", a, b))
    rand = {d: (rng.random((h, w)) < d, rng.random((h, w)) < d) for d in (0.05, 0.5, 0.95)}
    out.append(("full-full", full, full.copy()))
    out.append(("full-random", full, rand[0.5][1]))
    some = rand[0.5][0] | (yy + xx == 0)                                  # not empty even on a 1 x 1 plane
    out.append(("empty-prediction", empty, some))
    out.append(("empty-target", some, empty))
    out.append(("both-empty", empty, empty.copy()))
    out.append(("identical", some, some.copy()))
    a, b = empty.copy(), empty.copy()
    a[:min(3, h), :min(3, w)] = True
    b[max(h - 3, 0):, max(w - 3, 0):] = True
    out.append(("blobs", a, b))                                            # the largest d2 the plane allows
    out.append(("checkerboards", (yy + xx) % 2 == 0, (yy + xx) % 2 == 1))  # every on pixel a contour pixel
    for d, (a, b) in rand.items():
        out.append((f"random{d}", a, b))
    r = max(min(h, w) // 3, 1)
    out.append(("ring-disc", _disc(h, w, r) & ~_disc(h, w, max(r - 2, 0)), _disc(h, w, r)))
    return out


@functools.lru_cache(maxsize=None)
def _planes(h, w):
    """Per family of an h x w plane: (logits, target, {pct: (stats, sums)} filled on demand).  Computed once, never modified."""
    rng = np.random.default_rng(h * 1009 + w)
    planes = []
    for name, a, b in _families(h, w, seed=h * 31 + w):
        x, t = _encode(a, ON_LOGITS, OFF_LOGITS, rng), _encode(b, ON_TARGETS, OFF_TARGETS, rng)
        assert np.array_equal(R.pred_on(x), a) and np.array_equal(R.target_on(t), b), name
        planes.append((name, x, t, {}))
    return planes


def _want(plane, pct):
    name, x, t, cache = plane
    if pct not in cache:
        cache[pct] = R.plane_stats(R.pred_on(x), R.target_on(t), pct)
    return cache[pct]


def _batch(n, c, h, w, pct, start=0):
    planes = _planes(h, w)
    picks = [planes[(start + i) % len(planes)] for i in range(n * c)]
    x = np.stack([p[1] for p in picks]).reshape(n, c, h, w)
    t = np.stack([p[2] for p in picks]).reshape(n, c, h, w)
    stats = np.stack([_want(p, pct)[0] for p in picks]).reshape(n, c, 2, 4)
    sums = np.stack([_want(p, pct)[1] for p in picks]).reshape(n, c, 2)
    return torch.from_numpy(x), torch.from_numpy(t), torch.from_numpy(stats), torch.from_numpy(sums), [p[0] for p in picks]


def _close(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    print(f"{what} largest relative difference {float((err / np.maximum(np.abs(want), 1e-300)).max() if err.size and err.max() > 0 else 0.0):.3e}")
    assert np.all(err <= RTOL * np.abs(want)), (what, got, want)


def _raw_call(x, t, pct):
    """The C entry point on poisoned outputs: whatever the call leaves unwritten shows."""
    from glfusion_amd._lib import check, lib
    n, c, h, w = x.shape
    stats = torch.full((n, c, 2, 4), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device=DEV)
    sums = torch.full((n, c, 2), float("nan"), dtype=torch.float64, device=DEV)
    check(lib.glf_contour_distances(C.c_void_p(x.data_ptr()), C.c_void_p(t.data_ptr()), C.c_void_p(stats.data_ptr()), C.c_void_p(sums.data_ptr()),
                                    n, c, h, w, pct, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "contour_distances")
    return stats, sums


SHAPES = [(n, c, h, w) for (h, w) in [(1, 1), (1, 7), (7, 1), (5, 9), (67, 45), (112, 112)] for (n, c) in [(1, 1), (3, 5), (2, 8)]]


@pytest.mark.parametrize("n,c,h,w", SHAPES)
def test_kernel_equals_restatement(n, c, h, w):
    families = len(_planes(h, w))
    # (1, 1) walks every family, one launch each, on the small planes; the larger batches hold 15 or all 16 of the families at once
    starts = range(families) if (n, c) == (1, 1) else [h % families]
    for start in starts:
        x, t, want_stats, want_sums, names = _batch(n, c, h, w, 95, start)
        stats, sums = _raw_call(x.to(DEV), t.to(DEV), 95)
        assert torch.equal(stats.cpu(), want_stats), (names, stats.cpu().tolist(), want_stats.tolist())
        _close(sums.cpu().numpy(), want_sums.numpy(), f"{n}x{c}x{h}x{w} {names[0]}.. sum_d")
        empty = (want_stats[..., 0, 0] == 0) | (want_stats[..., 1, 0] == 0)
        assert bool((sums.cpu()[empty] == 0.0).all()) and bool((stats.cpu()[empty][..., 1:] == -1).all())


def test_kernel_on_224_planes():
    """Past one column strip and past the 64 KB a plane of 16-bit row distances would take: a full checkerboard (25 088 contour
    pixels, every on pixel one) against a shifted checkerboard confined to the 32 rightmost columns, so d2 runs from 1 to ~190^2."""
    from glfusion_amd import data
    h = w = 224
    yy, xx = np.mgrid[:h, :w]
    a, b = (yy + xx) % 2 == 0, ((yy + xx) % 2 == 1) & (xx >= w - 32)
    rng = np.random.default_rng(224)
    x, t = _encode(a, ON_LOGITS, OFF_LOGITS, rng)[None, None], _encode(b, ON_TARGETS, OFF_TARGETS, rng)[None, None]
    want_stats, want_sums = R.stats_ref(x, t, 95)
    stats, sums = data.contour_stats(torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV))
    assert int(want_stats[0, 0, 0, 0]) == 25088 and int(want_stats[0, 0, 0, 1]) > 180 ** 2
    assert torch.equal(stats.cpu(), torch.from_numpy(want_stats)), (stats.cpu().tolist(), want_stats.tolist())
    _close(sums.cpu().numpy(), want_sums, "224x224 sum_d")


@pytest.mark.parametrize("pct", [0, 50, 95, 100])
def test_percentiles(pct):
    from glfusion_amd import data
    x, t, want_stats, want_sums, names = _batch(2, 8, 67, 45, pct, start=1)
    stats, sums = data.contour_stats(x.to(DEV), t.to(DEV), percentile=pct)
    assert torch.equal(stats.cpu(), want_stats), (pct, names)
    _close(sums.cpu().numpy(), want_sums.numpy(), f"pct {pct} sum_d")


@pytest.mark.parametrize("pct", [0, 95, 100])
def test_rank_edges(pct):
    """Source contours of exactly 1, 2, 21 and 22 pixels: pct * (count - 1) divisible by 100 (1, 21) and not (2, 22)."""
    from glfusion_amd import data
    h, w = 9, 45
    rng = np.random.default_rng(5)
    target = np.zeros((h, w), bool)
    target[4:8, 3:30] = rng.random((4, 27)) < 0.6
    target[6, 40] = True
    xs, ts = [], []
    for k in (1, 2, 21, 22):
        a = np.zeros((h, w), bool)
        a[0, 0:2 * k:2] = True                                                # k isolated pixels: each its own contour
        assert int(R.contour(a).sum()) == k
        xs.append(_encode(a, ON_LOGITS, OFF_LOGITS, rng))
        ts.append(_encode(target, ON_TARGETS, OFF_TARGETS, rng))
    x, t = np.stack(xs)[None], np.stack(ts)[None]                            # [1, 4, h, w]
    want_stats, want_sums = R.stats_ref(x, t, pct)
    assert want_stats[0, :, 0, 0].tolist() == [1, 2, 21, 22]
    if pct == 95:
        assert (want_stats[0, 1:, 0, 2] != want_stats[0, 1:, 0, 3]).any()    # the two ranks do pick different values somewhere
    stats, sums = data.contour_stats(torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV), percentile=pct)
    assert torch.equal(stats.cpu(), torch.from_numpy(want_stats)), (stats.cpu().tolist(), want_stats.tolist())
    _close(sums.cpu().numpy(), want_sums, f"rank edges pct {pct}")
    m = data.contour_metrics(stats, sums, percentile=pct)
    want = R.metrics_ref(want_stats, want_sums, pct)
    _close(m["hdp"].cpu().numpy(), want["hdp"], f"rank edges pct {pct} hdp")


def test_two_calls_are_bitwise_equal():
    from glfusion_amd import data
    x, t, _, _, _ = _batch(3, 5, 112, 112, 95, start=2)
    x, t = x.to(DEV), t.to(DEV)
    s1, d1 = data.contour_stats(x, t)
    s2, d2 = data.contour_stats(x, t)
    assert torch.equal(s1, s2) and torch.equal(d1.view(torch.int64), d2.view(torch.int64))


def test_stream_order():
    """Issued behind kernels that write its input on the same non-default stream, the call sees that input."""
    from glfusion_amd import data
    x, t, want_stats, want_sums, _ = _batch(3, 5, 67, 45, 95, start=3)
    x_dev, t_dev = x.to(DEV), t.to(DEV)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        buf = torch.full_like(x_dev, -7.0)                                  # every pixel off until the copies below have run
        tmp = x_dev
        for _ in range(8):
            tmp = tmp.clone()
        buf.copy_(tmp)
        stats, sums = data.contour_stats(buf, t_dev)
    stream.synchronize()
    assert torch.equal(stats.cpu(), want_stats)
    _close(sums.cpu().numpy(), want_sums.numpy(), "stream order sum_d")


def test_contour_metrics_equal_restatement():
    from glfusion_amd import data
    x, t, want_stats, want_sums, names = _batch(2, 8, 67, 45, 95, start=0)
    stats, sums = data.contour_stats(x.to(DEV), t.to(DEV))
    m = data.contour_metrics(stats, sums)
    want = R.metrics_ref(want_stats.numpy(), want_sums.numpy())
    masks = torch.stack([m[k] for k in ("scored", "missed", "spurious", "absent")])
    assert masks.dtype == torch.bool and bool((masks.sum(dim=0) == 1).all())  # exactly one per pair
    for k in ("scored", "missed", "spurious", "absent"):
        assert np.array_equal(m[k].cpu().numpy(), want[k]), k
        assert bool(want[k].any()), k                                          # the batch holds every kind of pair
    scored = want["scored"]
    for k in ("hd", "hdp", "assd"):
        assert m[k].dtype == torch.float64 and tuple(m[k].shape) == (2, 8)
        _close(m[k].cpu().numpy()[scored], want[k][scored], k)
    acc = data.ContourAccumulator(8, DEV)
    acc += (x.to(DEV), t.to(DEV))
    acc += (x.to(DEV), t.to(DEV))
    _check_report(acc.report(), R.report_ref([(x.numpy(), t.numpy())] * 2))


def _check_report(got, want):
    assert set(got) == {"hd", "hd95", "assd", "scored", "missed", "spurious", "absent", "mean"}
    for k in ("scored", "missed", "spurious", "absent"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("hd", "hd95", "assd"):
        assert [x is None for x in got[k]] == [x is None for x in want[k]], (k, got[k], want[k])
        _close([x for x in got[k] if x is not None], [x for x in want[k] if x is not None], f"report {k}")
    assert (got["mean"] is None) == (want["mean"] is None)
    if want["mean"] is not None:
        _close(got["mean"], want["mean"], "report mean")


def _shape_of(lines):
    """Printed lines with every number masked: the format of a pass's output, whatever the last digit of a loss is."""
    return [re.sub(r"-?\d+\.\d+(e-?\d+)?", "#", line) for line in lines]


def _trainer(tmp_path, views, **train):
    from glfusion_amd.engine import Trainer
    from oracle import glfusion_ref as orc
    cfg = {"train": {"batch_size": 1, "num_epochs": 1, "clip_length": 3, "view_num": list(views), "test_view": list(views),
                     "save_dir": str(tmp_path), "iters_per_epoch": 1, "global_rank": 0, "validate_every_epoch": False, **train},
           "net": {"opt": {"opt_name": "Adam", "lr": 3e-4, "params": (0.9, 0.999), "weight_decay": 1e-5}}}
    t = Trainer(cfg)
    ref = orc.Global_and_Local(list(views))
    orc.closed_form_fill(ref, salt=9)                                          # predictions that overlap the parts (test_gpu_data.py)
    t.model.load_state_dict(ref.state_dict(), strict=True)
    return t


def test_trainer_eval_reports_contour_metrics(tmp_path, capsys):
    from glfusion_amd.data import SyntheticPatients
    views = ["1", "4"]
    patients = SyntheticPatients(views, 1, clip_length=3, h0=150, w0=170, device=DEV, seed=5)
    t = _trainer(tmp_path, views, contour_metrics=True)
    seen = {v: [] for v in views}
    capsys.readouterr()
    t.eval(patients=patients, on_clip=lambda k, v, logits, masks: seen[v].append((k, logits.cpu().numpy().copy(), masks.cpu().numpy().copy())))
    out_on = capsys.readouterr().out.splitlines()
    rep = t.eval_report["contour"]
    assert set(rep) == set(views) and all(len(seen[v]) == 1 and seen[v][0][0] == 0 for v in views)
    for v in views:
        want = R.report_ref([(x, m) for _, x, m in seen[v]])
        assert all(len(rep[v][k]) == 5 for k in ("hd", "hd95", "assd", "scored", "missed", "spurious", "absent"))
        _check_report(rep[v], want)
        assert [a + b + c + d for a, b, c, d in zip(rep[v]["scored"], rep[v]["missed"], rep[v]["spurious"], rep[v]["absent"])] == [3] * 5
    # view '1' shows channels 3 and 1 only: its other parts are never scored, and report None
    assert all(rep["1"]["scored"][c] == 0 and rep["1"]["hd"][c] is None for c in (0, 2, 4))
    assert sum(sum(rep[v]["scored"]) for v in views) > 0                       # the fixture is not degenerate
    assert len(out_on) == 2 * len(views) and sum("contour (pixels)" in line for line in out_on) == len(views)
    # option off: the parent behaviour's report and lines, nothing more
    t.contour_metrics = False
    capsys.readouterr()                                                        # drop what the comparisons above printed
    t.eval(patients=patients)
    out_off = capsys.readouterr().out.splitlines()
    assert "contour" not in t.eval_report and set(t.eval_report) == {"loss", "part_dice"}
    assert _shape_of(out_off) == _shape_of([line for line in out_on if "contour (pixels)" not in line])
    assert len(out_off) == len(views) and all(line.startswith(f"validation view {v}: loss ") for line, v in zip(out_off, views))


def test_validation_and_test_reports_contour_metrics(tmp_path, capsys, monkeypatch):
    import random
    from glfusion_amd import data
    infos = data.synthetic_infos(["4"], 2, clip_length=6, device="cpu", seed=2)
    t = _trainer(tmp_path, ["4"], contour_metrics=True, clip_length=6)
    seen = []
    add = data.ContourAccumulator.add

    def recording_add(self, logits, target):
        seen.append((logits.cpu().numpy().copy(), target.cpu().numpy().copy()))
        return add(self, logits, target)

    monkeypatch.setattr(data.ContourAccumulator, "add", recording_add)
    random.seed(3)
    capsys.readouterr()
    t.validation_and_test(net_root=None, infos=infos, val_list=("0_0",), test_list=("0_1",), reduce=False)
    lines = capsys.readouterr().out.splitlines()
    assert len(seen) == 2                                                      # one clip per split, one launch per (view, clip)
    for (name, clip) in zip(("Inner-val", "Inner-test"), seen):
        res = t.validation_report[name]["4"]
        assert set(res) == {"metrics", "loss", "part_dice", "contour"}
        _check_report(res["contour"], R.report_ref([clip]))
    assert sum(sum(t.validation_report[s]["4"]["contour"]["scored"]) for s in ("Inner-val", "Inner-test")) > 0
    assert len(lines) == 4 and sum("contour (pixels)" in line for line in lines) == 2
    monkeypatch.setattr(data.ContourAccumulator, "add", add)
    t.contour_metrics = False
    random.seed(3)
    capsys.readouterr()                                                        # drop what the comparisons above printed
    t.validation_and_test(net_root=None, infos=infos, val_list=("0_0",), test_list=("0_1",), reduce=False)
    off_lines = capsys.readouterr().out.splitlines()
    assert _shape_of(off_lines) == _shape_of([line for line in lines if "contour (pixels)" not in line])
    assert all("contour" not in t.validation_report[s]["4"] for s in ("Inner-val", "Inner-test"))
