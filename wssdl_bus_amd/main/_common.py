"""What the three command lines share: the reference's flags (code/main/*.py) and the set-up before the call."""
import argparse
import pprint

import numpy as np
import torch

from ..fast_rcnn.config import cfg, cfg_from_list
from ..mil.core import MIL_FUNCS, parse_funcs


def train_parser(description, default_network):
    p = argparse.ArgumentParser(description=description)
    p.add_argument('--max_iters', help='maximum iterations', default=60000, type=int)
    p.add_argument('--s_start_iter', help='start iter. for supervised learning', default=0, type=int)
    p.add_argument('--s_end_iter', help='end iter. for supervised learning', default=60000, type=int)
    p.add_argument('--ws_start_iter', help='start iter. for weakly supervised learning', default=0, type=int)
    p.add_argument('--ws_end_iter', help='end iter. for weakly supervised learning', default=60000, type=int)
    p.add_argument('--pretrained_model', help='a snapshot of this package or a torch state_dict file (loaded non-strictly)',
                   default=None, type=str)
    p.add_argument('--resume', help='a snapshot of this package to continue from', default=None, type=str)
    p.add_argument('--randomize', help='randomize (do not use a fixed seed)', action='store_true')
    p.add_argument('--network', help='name of the network', default=default_network, type=str)
    p.add_argument('--net_depth', help='network depth', default=18, type=int)
    p.add_argument('--dataset', help='dataset', default='SNUBH', type=str)
    p.add_argument('--norm_type', help='normalization type', default='BN', type=str)
    p.add_argument('--opt', help='optimizer', default='adam', type=str)
    p.add_argument('--lr', help='initial learning rate', default=5e-04, type=float)
    p.add_argument('--lr_scheduling', help='how to change the learning rate during training', default='const', type=str)
    p.add_argument('--mil_funcs', metavar='NAME,NAME', default=None, type=parse_funcs,
                   help='bag functions of the MIL term: for bags labelled 1, for the others; each one of %s '
                        '(default: the wiring\'s own pair)' % ', '.join(MIL_FUNCS))
    p.add_argument('--imdb_train_s', help='supervised training set', default='bus_test', type=str)
    p.add_argument('--imdb_train_ws', help='weakly supervised training set', default='bus_test', type=str)
    p.add_argument('--imdb_test', help='test set', default='bus_test', type=str)
    p.add_argument('--output_dir', help='output path', required=True, type=str)
    p.add_argument('--val_ims_per_batch', help='images per validation forward', default=1, type=int)
    p.add_argument('--qual_res_off', help='turn off saving qualitative results', default=True, action='store_false')
    p.add_argument('--set_cfgs', help='set config keys', default=None, nargs=argparse.REMAINDER)
    return p


def setup(args, seed=True):
    print('Called with args:')
    print(args)
    if getattr(args, 'set_cfgs', None) is not None:
        cfg_from_list(args.set_cfgs)
    print('Using config:')
    pprint.pprint(cfg)
    if seed:
        np.random.seed(cfg.RNG_SEED)
        torch.manual_seed(cfg.RNG_SEED)


def run_training(args, train_fn):
    from ..datasets.factory_bus import get_imdb
    from ..fast_rcnn.train_bus import get_test_roidb, get_training_roidb
    from ..networks.factory_bus import get_network
    setup(args, not args.randomize)
    imdb_train_s = get_imdb(args.imdb_train_s)
    print('Loaded dataset `{:s}` for training'.format(imdb_train_s.name))
    roidb_train_s = get_training_roidb(imdb_train_s)
    imdb_train_ws = get_imdb(args.imdb_train_ws)
    print('Loaded dataset `{:s}` for training'.format(imdb_train_ws.name))
    roidb_train_ws = get_training_roidb(imdb_train_ws)
    imdb_test = get_imdb(args.imdb_test)
    print('Loaded dataset `{:s}` for test'.format(imdb_test.name))
    roidb_test = get_test_roidb(imdb_test)
    print('Output will be saved to `{:s}`'.format(args.output_dir))
    network = get_network(args.network, args.net_depth, args.dataset, args.norm_type).cuda().to(memory_format=torch.channels_last)
    network.train()
    print('Use network `{:s}` in training'.format(args.network))
    return train_fn(network, imdb_train_s, roidb_train_s, imdb_train_ws, roidb_train_ws, imdb_test, roidb_test, args.output_dir,
                    pretrained_model=args.pretrained_model, max_iters=args.max_iters, s_start_iter=args.s_start_iter,
                    s_end_iter=args.s_end_iter, ws_start_iter=args.ws_start_iter, ws_end_iter=args.ws_end_iter, opt=args.opt,
                    lr=args.lr, lr_scheduling=args.lr_scheduling, vis=args.qual_res_off, resume=args.resume,
                    val_ims_per_batch=args.val_ims_per_batch, mil_funcs=args.mil_funcs)
