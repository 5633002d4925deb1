"""RoIDataLayerJoint (reference roi_data_layer/layer_bus_joint.py): supervised and weak roidbs in one mini-batch."""
import numpy as np

from ..fast_rcnn.config import cfg
from .minibatch_bus import get_minibatch_joint


class RoIDataLayerJoint(object):
    """forward() -> the blobs of the next joint mini-batch: cfg.TRAIN.IMS_PER_BATCH supervised images first, then
    cfg.TRAIN.WS_IMS_PER_BATCH weak ones.  Index logic as the reference (:29-88): both permutations at construction
    (supervised first), each again whenever its next batch would run past the end, when training; np.arange order
    otherwise.  `rng` as in RoIDataLayer."""

    def __init__(self, roidb_s, roidb_ws, net_name, num_classes, is_training, rng=None):
        self._roidb_s = roidb_s
        self._roidb_ws = roidb_ws
        self._net_name = net_name
        self._num_classes = num_classes
        self._is_training = is_training
        self._rng = rng
        self._perm_s, self._cur_s = self._inds(len(roidb_s)), 0
        self._perm_ws, self._cur_ws = self._inds(len(roidb_ws)), 0

    def _inds(self, n):
        if self._is_training:
            return (self._rng or np.random).permutation(np.arange(n))
        return np.arange(n)

    def _get_next_minibatch_inds(self):
        if not cfg.TRAIN.HAS_RPN:
            raise NotImplementedError("only the cfg.TRAIN.HAS_RPN branch of the data layers exists")
        ns, nw = cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH
        if self._cur_s + ns > len(self._roidb_s):
            self._perm_s, self._cur_s = self._inds(len(self._roidb_s)), 0
        db_inds_s = self._perm_s[self._cur_s:self._cur_s + ns]
        self._cur_s += ns
        if self._cur_ws + nw > len(self._roidb_ws):
            self._perm_ws, self._cur_ws = self._inds(len(self._roidb_ws)), 0
        db_inds_ws = self._perm_ws[self._cur_ws:self._cur_ws + nw]
        self._cur_ws += nw
        return db_inds_s, db_inds_ws

    def state_dict(self):
        """Both permutations and cursors: what the next index draws depend on (besides the RNG stream's own state)."""
        return dict(perm_s=np.array(self._perm_s, dtype=np.int64), cur_s=int(self._cur_s),
                    perm_ws=np.array(self._perm_ws, dtype=np.int64), cur_ws=int(self._cur_ws))

    def load_state_dict(self, state):
        perm_s, perm_ws = np.array(state["perm_s"], dtype=np.int64), np.array(state["perm_ws"], dtype=np.int64)
        if perm_s.shape != (len(self._roidb_s),) or perm_ws.shape != (len(self._roidb_ws),):
            raise ValueError("data-layer state of %d + %d entries, these roidbs have %d + %d"
                             % (perm_s.size, perm_ws.size, len(self._roidb_s), len(self._roidb_ws)))
        self._perm_s, self._cur_s = perm_s, int(state["cur_s"])
        self._perm_ws, self._cur_ws = perm_ws, int(state["cur_ws"])

    def forward(self):
        picked_s, picked_ws = self._get_next_minibatch_inds()
        return get_minibatch_joint([self._roidb_s[i] for i in picked_s], [self._roidb_ws[i] for i in picked_ws],
                                   self._net_name, self._num_classes, self._is_training, rng=self._rng)
