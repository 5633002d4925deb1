"""python -m wssdl_bus_amd.main.test: the test protocol (reference code/main/test.py) -- an argument parser over
fast_rcnn.eval_batch.evaluate_images.  The per-image result pictures go to <output_dir>/test unless --qual_res_off."""
import argparse
import os

import torch

from ._common import setup


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Test a Faster R-CNN network')
    p.add_argument('--network', help='name of the network', default='Resnet_train', type=str)
    p.add_argument('--net_depth', help='network depth (only for ResNet [18, 34, 50, 101])', default=101, type=int)
    p.add_argument('--norm_type', help='normalization type (only for ResNet)', default='BN', type=str)
    p.add_argument('--trained_model', help='a snapshot of this package or a torch state_dict file', required=True, type=str)
    p.add_argument('--dataset', help='dataset', default='SNUBH', type=str)
    p.add_argument('--imdb_test', help='test set', default='bus_test', type=str)
    p.add_argument('--comp_mode', help='competition mode (accepted; no result files are written here)', action='store_true')
    p.add_argument('--output_dir', help='where <output_dir>/test/*.png go (default: next to the model)', default=None, type=str)
    p.add_argument('--batch_size', help='images per forward', default=8, type=int)
    p.add_argument('--qual_res_off', help='turn off saving qualitative results', default=True, action='store_false')
    p.add_argument('--set_cfgs', help='set config keys', default=None, nargs=argparse.REMAINDER)
    return p.parse_args(argv)


def main(argv=None):
    from ..datasets.factory_bus import get_imdb
    from ..fast_rcnn import snapshot
    from ..fast_rcnn.eval_batch import evaluate_images
    from ..fast_rcnn.train_bus import get_test_roidb
    from ..networks.factory_bus import get_network
    from ..roi_data_layer.minibatch_bus import entry_plane
    args = parse_args(argv)
    setup(args, seed=False)
    imdb = get_imdb(args.imdb_test)
    roidb = get_test_roidb(imdb)
    network = get_network(args.network, args.net_depth, args.dataset, args.norm_type).cuda().to(memory_format=torch.channels_last)
    snapshot.load_pretrained(network, args.trained_model)
    network.eval()
    out = args.output_dir or os.path.dirname(os.path.abspath(args.trained_model))
    vis_dir = os.path.join(out, 'test') if args.qual_res_off else None
    result = evaluate_images(network, [entry_plane(e) for e in roidb], [dict(boxes=e['boxes'], gt_classes=e['gt_classes']) for e in roidb],
                             type(network).__name__, batch_size=args.batch_size, classes=imdb.classes, vis_dir=vis_dir,
                             image_paths=[imdb.image_path_at(i) for i in range(len(roidb))])
    print('AP per class: %s, mean AP: %.4f' % (['%.4f' % a for a in result['aps']], result['mean_ap']))
    print('corloc: %s' % ['%.4f' % c for c in result['corloc_list']])
    return result


if __name__ == '__main__':
    main()
