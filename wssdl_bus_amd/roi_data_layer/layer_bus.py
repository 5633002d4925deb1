"""RoIDataLayer (reference roi_data_layer/layer_bus.py): mini-batches of one roidb, supervised or weak."""
import numpy as np

from ..fast_rcnn.config import cfg
from .minibatch_bus import get_minibatch


class RoIDataLayer(object):
    """forward() -> the blobs of the next mini-batch (device tensors).  The index logic is the reference's (:26-63):
    a permutation at construction and whenever the next batch would run past the end when training, np.arange
    order otherwise.  `rng`: a RandomState for the permutations and the mini-batch's draws (default: NumPy's global
    legacy stream, like the reference)."""

    def __init__(self, roidb, net_name, num_classes, is_training, is_ws, rng=None):
        self._roidb = roidb
        self._net_name = net_name
        self._num_classes = num_classes
        self._is_training = is_training
        self._is_ws = is_ws
        self._rng = rng
        self._ims_per_batch = cfg.TRAIN.WS_IMS_PER_BATCH if is_ws else cfg.TRAIN.IMS_PER_BATCH
        self._reset_inds()

    def _reset_inds(self):
        if self._is_training:
            self._perm = (self._rng or np.random).permutation(np.arange(len(self._roidb)))
        else:
            self._perm = np.arange(len(self._roidb))
        self._cur = 0

    def _get_next_minibatch_inds(self):
        if not cfg.TRAIN.HAS_RPN:
            raise NotImplementedError("only the cfg.TRAIN.HAS_RPN branch of the data layers exists")
        n = self._ims_per_batch
        if self._cur + n > len(self._roidb):                    # the batch would run past the end: start over
            self._reset_inds()
        start, self._cur = self._cur, self._cur + n
        return self._perm[start:start + n]

    def state_dict(self):
        """The permutation and the cursor: what the next index draws depend on (besides the RNG stream's own state)."""
        return dict(perm=np.array(self._perm, dtype=np.int64), cur=int(self._cur))

    def load_state_dict(self, state):
        perm = np.array(state["perm"], dtype=np.int64)
        if perm.shape != (len(self._roidb),):
            raise ValueError("data-layer state of %d entries, this roidb has %d" % (perm.size, len(self._roidb)))
        self._perm, self._cur = perm, int(state["cur"])

    def forward(self):
        picked = self._get_next_minibatch_inds()
        return get_minibatch([self._roidb[i] for i in picked], self._net_name, self._num_classes, self._is_training,
                             self._is_ws, rng=self._rng)
