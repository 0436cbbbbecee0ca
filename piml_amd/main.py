# -*- coding: utf-8 -*-
"""Experiment driver with the reference's command line (src/main.py:26-173): pre-train PINNSF
pointwise, optionally fine-tune it through differentiable rollouts (-f), then roll a clip out and
count collisions -- the pairwise operators AND the PINNSF networks (incl. their train-mode dropout) on this
package's hand-written gfx950 kernels; PyTorch-ROCm is the plumbing (memory, streams, autograd, Adam).

    python -m piml_amd.main [--flags as in the reference]

Flag names and defaults are the reference's, except `--device` (default `cuda`: there is no CPU
path) and the data YAMLs (shipped under piml_amd/configs/, paths relative to the YAML).  Fixes of
reference driver bugs: fine-tuning uses `--ft_batch_size` (main.py:153 reads an
undefined `args.f_batch_size`) on channelled windows, and does not need a checkpoint on disk.
"""
import argparse
import os

os.environ.setdefault('DEBUG_CLR_GRAPH_PACKET_CAPTURE', '0')      # before torch brings the HIP runtime up (piml_amd.hip_graphs_safe)
import random
import string
import time

import numpy as np
import torch

from .data import dataset as DATASET
from .functions import metrics as METRIC
from .models import simulators as SIMULATOR
from .utils import data_loader as LOADER

_CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'configs', 'data_configs')


def get_args(argv=None):
    p = argparse.ArgumentParser(description='AI pedestrian simulation')
    A = p.add_argument
    A('--exp_name', type=str, default='pedsim_debug'); A('--user_name', type=str, default='guozhen')
    A('--seed', type=int, default=666); A('-f', '--finetune_flag', action='store_true')
    A('--data_config', type=str, default=os.path.join(_CFG, 'toy.yaml'))
    A('--ft_data_config', type=str, default=os.path.join(_CFG, 'toy_f.yaml'))
    A('--vis_data_config', type=str, default=os.path.join(_CFG, 'data_vis.yaml'))
    A('--model', type=str, default='pinnsf_m'); A('--device', type=str, default='cuda')
    A('--gpus', type=str, default='3'); A('--learning_rate', type=float, default=0.002)
    A('--batch_size', type=int, default=3); A('--ft_batch_size', type=int, default=4)
    A('--shuffle', action='store_true'); A('--num_workers', type=int, default=0)
    A('--weight_decay', type=float, default=5e-4); A('--epochs', type=int, default=2)
    A('--dropout', type=float, default=0.5); A('--n_embedding', type=int, default=10)
    A('--hidden_size', type=int, default=32); A('--activation', type=str, default='relu')
    A('--patience', type=int, default=1); A('--ft_patience', type=int, default=5)
    A('--topk_ped', type=int, default=6); A('--topk_obs', type=int, default=10)
    A('--sight_angle_ped', type=int, default=90); A('--sight_angle_obs', type=int, default=90)
    A('--dist_threshold_ped', type=int, default=4); A('--dist_threshold_obs', type=int, default=4)
    A('--train_ratio', type=float, default=0.6); A('--val_ratio', type=float, default=0.2)
    A('--test_ratio', type=float, default=0.2)
    A('--encoder_hidden_size', type=int, default=128); A('--processor_hidden_size', type=int, default=128)
    A('--decoder_hidden_size', type=int, default=64); A('--encoder_hidden_layers', type=int, default=3)
    A('--processor_hidden_layers', type=int, default=16); A('--decoder_hidden_layers', type=int, default=2)
    A('--add_noise_flag', action='store_true'); A('--add_noise_std', type=float, default=0.05)
    A('--correction_hidden_layers', type=int, default=1); A('--finetune_lr_decay', type=float, default=1)
    A('--finetune_wd_aug', type=int, default=1); A('--num_history_velocity', type=int, default=1)
    A('--skip_frames', type=int, default=25); A('--valid_steps', type=int, default=5)
    A('--time_decay', type=float, default=1); A('--training_mode', type=str, default='normal')
    A('--res_hidden_layers', type=int, default=3); A('--ft_lr_decay2', type=float, default=0.)
    A('--save_configs', action='store_true'); A('--reg_weight', type=float, default=0.)
    A('--collision_threshold', type=float, default=0.5); A('--collision_loss_weight', type=float, default=10)
    A('--val_coll_weight', type=float, default=30); A('--hard_collision_penalty', type=float, default=10)
    A('--metrics_impl', type=str, default='torch', choices=('torch', 'hip'))   # evaluation OT / MMD: batched torch | HIP kernels
    A('--teacher_weight', type=float, default=0); A('--collision_pred_weight', type=float, default=10)
    A('--collision_focus_weight', type=float, default=10); A('--new_collision_loss_flag', type=int, default=0)
    A('--tags', type=str, default=''); A('--iter_flag', type=int, default=0)
    A('--iter_model_name_suffix', type=str, default=''); A('--pinnsf_interaction', type=str, default='sim')
    A('--dataset_name', type=str, default='ucy'); A('--true_label_weight', type=float, default=0)
    A('--collision_loss_version', type=str, default='v0')
    A('--save_dir', type=str, default='', help='checkpoint directory ("" = keep weights in memory only)')
    A('--tunableop', type=int, default=0, help='1: load the pre-tuned GEMM selections (piml_amd/tuning)')
    A('--hip_graph', type=int, default=1, help='0: run the training steps (pointwise pre-training and fine-tuning) eagerly instead of replaying captured HIP graphs')
    A('--inplace_quirk', type=int, default=1,
      help='1 (default): carry the waypoint indices / first-frame velocity history of a rollout over to the next rollout of '
           'the same clip or batch, as the reference does through its in-place views (SURVEY quirk Q12); 0: every '
           'rollout starts from the untouched data')
    A('--library_gemm', type=int, default=0,
      help='1: run the networks on library GEMMs + HIP glue kernels instead of the fused matrix-core kernels.  Both are '
           'float32 and agree to 1e-5 per step (tests/test_ucy_gpu.py); over a whole training run a hidden unit waking up '
           'one batch earlier in one of them shifts the trajectory (DESIGN.md section 2).  The library path happens to '
           'round like the reference\'s CPU GEMM and reproduces its printed UCY numbers to 1e-6: use it to REPRODUCE a '
           'reference run digit for digit, the default (0) to train fast')
    A('--fix_dest_norm', action='store_true',
      help='desired-force direction normalised per agent for channelled (C, N, 7) input too; the reference reduces '
           'over dim=1 = the AGENT axis there (src/models/model.py:1290, SURVEY quirk Q2), which stays the default')
    args = p.parse_args(argv)
    args.model_name_suffix = ''.join(random.sample(list(string.ascii_lowercase) + list(string.digits), 8))
    return args


def set_exp_configs(args):
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(args.seed)
        from . import ops
        # the fused kernels' own draw counter back to 0 (a repeated seed does not rewind it by itself), on the run's device
        ops.dropout_seed(args.seed, getattr(args, 'device', None) if str(getattr(args, 'device', '')).startswith('cuda') else None)


LAST_RUN = {}      # the objects of the most recent main() call (tests / notebooks): simulator, histories, args


def main(argv=None, init_state=None):
    """`init_state`: optional state_dict loaded into the freshly built pre-training network (parity tests start
    from the reference's own initial weights; parameter initialisation consumes the RNG in a different order)."""
    args = get_args(argv)
    set_exp_configs(args)
    if args.library_gemm:
        import piml_amd.models.model as _M
        _M.FUSED_ENCODER = _M.FUSED_NETWORK = _M.FUSED_ROW_DECODER = _M.FUSED_KSUM_TAIL = False
    if args.tunableop:
        from . import tuning
        print('pre-tuned GEMM selections loaded:', tuning.load())
    start_time = time.time()

    synthetic = DATASET.PointwisePedDataset()
    synthetic.load_data(args.data_config)
    print('number of training dataset: ', len(synthetic.raw_data['train']))
    synthetic.build_dataset(args)
    loaders = LOADER.data_loader(synthetic.train_data, args.batch_size, args.seed, shuffle=args.shuffle, drop_last=True)
    simulator = SIMULATOR.BaseSimulator(args)
    if init_state is not None:
        simulator.model.load_state_dict(init_state)
    history = simulator.train(loaders, synthetic.valid_data)
    LAST_RUN.clear()
    LAST_RUN.update(args=args, simulator=simulator, pretrain_history=list(history), finetune_history=[], n_train=len(synthetic.train_data))
    if hasattr(synthetic, 'test_data'):
        simulator.test_multiple_rollouts(synthetic.test_data, load_model=False)

    if args.finetune_flag:
        real = DATASET.TimeIndexedPedDataset2()
        real.load_data(args.ft_data_config)
        real.build_dataset(args)
        ft_loaders = LOADER.data_loader(real.train_data, args.ft_batch_size, args.seed, shuffle=args.shuffle, drop_last=True)
        ft_history = simulator.finetune(ft_loaders, real.valid_data, real.test_data)
        LAST_RUN.update(finetune_history=ft_history, finetune_data=real)
        history += ft_history
    print('Total train time: {}'.format(time.time() - start_time))

    vis = DATASET.TimeIndexedPedDatasetforVis()
    vis.load_data(args.vis_data_config)
    vis.build_dataset(args)
    results = []
    with torch.no_grad():
        simulator.model.eval()
        for d in vis.dataset['vis']:
            out = simulator.get_multiple_rollouts(d, load_model=False)
            soft = METRIC.collision_count(out.position, 0.5, reduction='sum')
            hard = METRIC.collision_count(out.position, 0.5 / 2, reduction='sum')
            print('#collisions soft/hard: {} / {}'.format(soft, hard))
            results.append((soft, hard))
    return history, results


if __name__ == '__main__':
    main()
