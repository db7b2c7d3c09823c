"""What the contour metrics cost (profiles/contour_metrics.txt).

  python profiles/ubench/contour_metrics.py eval [repeats]      Trainer.eval on the default synthetic patients, option off and on
  python profiles/ubench/contour_metrics.py kernel [repeats]    glf_contour_distances alone at (40, 5, 112, 112)

`eval`: main.py's views (1, 3, 4), 2 patients x 40 frames, host clock around a pass that ends in a device synchronise; off and on
alternate.  Run from a checkout of the parent commit (which has no option) it times the pass as it was: the off figure must agree
with that within the spread.  `kernel`: device events around groups of 20 calls on the model's own predictions for one (patient,
view) and on the worst case, a checkerboard against the shifted checkerboard (every on pixel a contour pixel)."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

VIEWS = ["1", "3", "4"]


def _trainer(**train):
    from glfusion_amd.engine import Trainer
    cfg = {"train": {"batch_size": 1, "num_epochs": 1, "clip_length": 40, "view_num": VIEWS, "test_view": VIEWS, "save_dir": "./result/ckpt",
                     "iters_per_epoch": 1, "global_rank": 1, **train},           # global_rank 1: nothing printed by the pass
           "net": {"opt": {"opt_name": "Adam", "lr": 3e-4, "params": (0.9, 0.999), "weight_decay": 1e-5}}}
    return Trainer(cfg)


def _timed_eval(t):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t.eval()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _line(tag, ms):
    return f"{tag:<34}: median {statistics.median(ms):8.2f} ms  (min {min(ms):.2f}, max {max(ms):.2f}; {len(ms)} passes)"


def run_eval(repeats: int) -> None:
    from glfusion_amd import data
    t = _trainer()
    has_option = hasattr(data, "contour_stats")
    modes = [False, True] if has_option else [False]
    for on in modes:                                                              # warm up every shape of both passes
        t.contour_metrics = on
        _timed_eval(t)
    ms = {on: [] for on in modes}
    for _ in range(repeats):
        for on in modes:
            t.contour_metrics = on
            ms[on].append(_timed_eval(t))
    print(f"Trainer.eval, views {VIEWS}, 2 patients x 40 frames, 112 x 112, default precision")
    print(_line("contour_metrics off" if has_option else "no contour option (parent)", ms[False]))
    if has_option:
        print(_line("contour_metrics on", ms[True]))
        print(f"difference of the medians: {statistics.median(ms[True]) - statistics.median(ms[False]):.2f} ms per pass = 6 launches of "
              f"glf_contour_distances, their torch arithmetic and one host read")
        t.contour_metrics = True
        t.eval()
        for v in VIEWS:
            r = t.eval_report["contour"][v]
            print(f"view {v}: mean (hd, hd95, assd) {r['mean']}; scored {r['scored']} missed {r['missed']} spurious {r['spurious']} absent {r['absent']}")


def run_kernel(repeats: int) -> None:
    import torch
    from glfusion_amd import data
    t = _trainer()
    seen = []
    t.eval(on_clip=lambda k, v, logits, masks: seen.append((v, logits.clone(), masks.clone())))
    v, logits, masks = next(s for s in seen if s[0] == "4")
    yy, xx = torch.meshgrid(torch.arange(112, device="cuda"), torch.arange(112, device="cuda"), indexing="ij")
    board = ((yy + xx) % 2 == 0).float()
    cases = {f"model's predictions, view {v}": (logits, masks),
             "checkerboard vs shifted": ((board * 8 - 4).expand(40, 5, 112, 112).contiguous(), (1 - board).expand(40, 5, 112, 112).contiguous()),
             "all planes empty": (torch.full((40, 5, 112, 112), -4.0, device="cuda"), torch.zeros(40, 5, 112, 112, device="cuda"))}
    print("glf_contour_distances alone, [40][5][112][112], 400 workgroups of 1024 threads, device events around 20 calls")
    for name, (x, m) in cases.items():
        stats, _ = data.contour_stats(x, m)
        for _ in range(3):
            data.contour_stats(x, m)
        us = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                data.contour_stats(x, m)
            b.record()
            b.synchronize()
            us.append(a.elapsed_time(b) * 1e3 / 20)
        pixels = int(stats[..., 0].sum())
        print(f"{name:<32}: median {statistics.median(us):8.1f} us per call  (min {min(us):.1f}, max {max(us):.1f}; {repeats} groups); "
              f"{pixels} contour pixels in all, largest d2 {int(stats[..., 1].max())}")


if __name__ == "__main__":
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    if len(sys.argv) > 1 and sys.argv[1] == "eval":
        run_eval(n)
    elif len(sys.argv) > 1 and sys.argv[1] == "kernel":
        run_kernel(n)
    else:
        raise SystemExit(__doc__)
