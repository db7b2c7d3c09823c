#!/usr/bin/env python3
"""Entry point with the reference's surface (GLfusion/main.py:885-965): the same `config` dict keys, `--mode
{train,val,visual}`, `main(rank, config)`, `Trainer(config)` -- running the MI355X HIP engine on patient volumes (`--infos`, `--video-infos`,
`--train-list`: the reference's infos dicts and id list) or, without them, on synthetic clips (the reference's data files are not
shipped).  Multi-GPU: `python -m torch.distributed.run --nproc-per-node N main.py
--mode train` (one process per GPU, RCCL gradient all-reduce) instead of the reference's nn.DataParallel."""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch
import torch.distributed as dist


def main(rank, config):
    if "local_rank" not in config["train"]:
        config["train"]["local_rank"] = config["train"]["global_rank"] = rank
    config["train"]["device"] = torch.device("cuda", config["train"]["local_rank"])
    parser = argparse.ArgumentParser()
    parser.add_argument("--mode", type=str, required=True)
    parser.add_argument("--precision", type=str, default=None, choices=("f32", "bf16x6", "f16x3", "f16", "bf16"),
                        help="contraction precision (config['train']['precision']); default: the engine's")
    parser.add_argument("--fold-bn", action="store_true",
                        help="evaluation with BatchNorm folded into the convolutions (config['train']['fold_bn']; f16x3 / f16 only)")
    parser.add_argument("--fold-bn-s16", action="store_true",
                        help="the same under 16-bit storage (config['train']['fold_bn_s16']; bf16 only)")
    parser.add_argument("--opt", type=str, default=None, choices=("Adam", "SGD"),
                        help="optimizer branch of main.py:158-165 (config['net']['opt']['opt_name']); default: the config's")
    parser.add_argument("--resume", action="store_true",
                        help="continue from the latest checkpoint in config['train']['save_dir'] (config['train']['is_load']); "
                             "checkpoints then also hold the optimizer state (config['train']['save_optimizer'])")
    parser.add_argument("--clip-grad-norm", type=float, default=None, metavar="X",
                        help="clip every step by the global gradient norm X and skip steps with a non-finite one, on the device "
                             "(config['train']['clip_grad_norm']; inf = the guard alone); default: off")
    parser.add_argument("--model", type=str, default=None,
                        choices=("Global_and_Local", "Global_and_Local_cyc_nofusion", "Foreground_and_Background", "Global_and_Local_Temporal",
                                 "Global_and_Local_conv_merge", "Global_only", "Global_only_cyc_nofusion", "Local_only", "model19",
                                 "Global_and_Local_CPS", "baseline_unet", "multiview_unet", "early_fusion", "late_fusion", "MLP_fusion"),
                        help="the network (config['net']['model']); default: the config's, else Global_and_Local.  The nine ablation "
                             "variants of ours.py train like it (Global_and_Local_CPS supervises both of its networks).  The U-Net "
                             "baselines (ours.py:2416-2625) and the fusion baselines early_fusion / late_fusion / MLP_fusion "
                             "(ours.py:2251-2383, 1044-1107) return no fusion features and train without the cycle loss")
    parser.add_argument("--cps-weight", type=float, default=None, metavar="X",
                        help="weight of the cross pseudo supervision term of --model Global_and_Local_CPS: on the unlabelled clip each "
                             "network's hard prediction supervises the other (config['train']['cps_weight']); default: 0, off")
    parser.add_argument("--infos", type=str, default=None, metavar="NPY",
                        help="train from patient volumes: the reference's pickled infos dict of the labelled frames "
                             "(config['train']['infos']); default: synthetic batches")
    parser.add_argument("--video-infos", type=str, default=None, metavar="NPY",
                        help="the infos dict of the whole videos, the cycle term's clips (config['train']['video_infos']); "
                             "needed beside --infos unless the model trains without the cycle loss")
    parser.add_argument("--train-list", type=str, default=None, metavar="NPY",
                        help="array of the patient ids to train on, the reference's data_list/train_list.npy "
                             "(config['train']['train_list']); default: the datasets' own 80 %% split")
    parser.add_argument("--contour-metrics", action="store_true",
                        help="evaluation also reports Hausdorff distance, its 95th percentile and the average symmetric surface "
                             "distance per view and part, in pixels (config['train']['contour_metrics']); default: off")
    args = parser.parse_args()
    if args.infos:
        config["train"]["infos"] = args.infos
    if args.video_infos:
        config["train"]["video_infos"] = args.video_infos
    if args.train_list:
        import numpy as np
        config["train"]["train_list"] = np.load(args.train_list, allow_pickle=True).tolist()
    if args.model:
        config["net"]["model"] = args.model
    if args.opt:
        config["net"]["opt"]["opt_name"] = args.opt
    if args.clip_grad_norm is not None:
        config["train"]["clip_grad_norm"] = args.clip_grad_norm
    if args.cps_weight is not None:
        config["train"]["cps_weight"] = args.cps_weight
    if args.resume:
        config["train"]["is_load"] = config["train"]["save_optimizer"] = True
    if args.precision:
        config["train"]["precision"] = args.precision
    if args.contour_metrics:
        config["train"]["contour_metrics"] = True
    if args.fold_bn:
        config["train"]["fold_bn"] = True
    if args.fold_bn_s16:
        config["train"]["fold_bn_s16"] = True
    from glfusion_amd.engine import Trainer
    trainer = Trainer(config)
    if args.mode == "train":
        from glfusion_amd.engine import NO_FUSION_FEATURES
        trainer.train(is_backbone=False, is_cycle=trainer.model_name not in NO_FUSION_FEATURES)
    elif args.mode == "val":
        print(trainer.eval(net_path="./path/to/ckpt", is_fuse=True, raw_data=True))
    elif args.mode == "visual":
        trainer.test_visualize("glfusion_amd")
    else:
        raise SystemExit(f"--mode {args.mode}: unknown mode; the valid modes are train, val and visual")


if __name__ == "__main__":
    config = {
        "train": {
            "cudnn": True, "enable_GPUs_id": [0], "device_ids": [0], "batch_size": 8, "num_workers": 8,
            "num_epochs": 1, "clip_length": 40, "view_num": ["1", "3", "4"], "test_view": ["1", "3", "4"],
            "dense_cyc": False, "seg_parts": True, "record_params": False, "save_dir": "./result/ckpt",
            "log_dir": "./result/log_info/log_01", "data_list_path": "./", "use_data": ["rmyy"], "alpha": 0.8,
            "is_load": False,
            # build-only keys
            "iters_per_epoch": 2,
        },
        "net": {"opt": {"opt_name": "Adam", "lr": 3e-4, "step_size": 50, "params": (0.9, 0.999), "weight_decay": 1e-5},
                "opt_loss_weight": {"opt_name": "Adam", "lr": 1e-3, "step_size": 50, "params": (0.9, 0.999), "weight_decay": 1e-5}},
    }
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    config["train"]["world_size"] = world
    config["train"]["distributed"] = world > 1
    config["train"]["local_rank"], config["train"]["global_rank"] = local, rank
    if world > 1:
        torch.cuda.set_device(local)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world)
    main(local, config)
