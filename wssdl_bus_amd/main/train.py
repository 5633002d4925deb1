"""python -m wssdl_bus_amd.main.train: joint training (reference code/main/train.py) -- an argument parser over
fast_rcnn.train_bus.train_net.  --qual_res_off turns the per-image result pictures off (they are on by default)."""
from ..fast_rcnn.train_bus import train_net
from ._common import run_training, train_parser


def parser():
    return train_parser('Train a Faster R-CNN network on combined mini-batches', 'Resnet_train')


def main(argv=None):
    args = parser().parse_args(argv)
    return run_training(args, train_net)


if __name__ == '__main__':
    main()
