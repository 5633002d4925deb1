"""Multiple-instance (image-level) bag logits for the weakly supervised loss.

Reference: code/lib/mil/core.py:11-96.  Instances (RoIs) arrive grouped by image in
batch order; for each bag (image) a bag function turns the bag's instance rows into one logit row.
Four of the reference's five functions select an instance row (mal-max, ben-max, mass-max, disc-max),
the fifth pools (mean-ben: [0, mean of the class-1 logits, 0]).  The functions below are the host-side
restatement in PyTorch; the device op (csrc/mil.hip) takes all five by number.
"""
import torch


def get_mal_max_logit(cur_logits):
    """Row of the instance with the largest malignant (class 2) logit (core.py:60-69)."""
    return cur_logits[torch.argmax(cur_logits[:, 2])].unsqueeze(0)


def get_ben_max_logit(cur_logits):
    """Row of the instance with the largest benign (class 1) logit (core.py:49-57)."""
    return cur_logits[torch.argmax(cur_logits[:, 1])].unsqueeze(0)


def get_mass_max_logit(cur_logits):
    """Row of the instance with the smallest background (class 0) logit (core.py:88-96)."""
    return cur_logits[torch.argmin(cur_logits[:, 0])].unsqueeze(0)


def get_disc_max_logit(cur_logits):
    """Row of the instance with the largest non-background logit (core.py:78-86)."""
    return cur_logits[torch.argmax(cur_logits[:, 1:].max(dim=1).values)].unsqueeze(0)


def get_mean_ben_logit(cur_logits):
    """[0, mean of the benign (class 1) logits, 0] (core.py:71-74): the one bag function that pools instead of
    selecting a row, so its gradient reaches every instance of the bag.  Classes beyond the reference's three are 0
    like class 0 and 2."""
    onehot = torch.zeros((1, cur_logits.shape[1]), dtype=cur_logits.dtype, device=cur_logits.device)
    onehot[0, 1] = 1.0
    return cur_logits[:, 1].mean() * onehot


def get_bag_logit(instance_logits, batch_inds, num_classes, bag_labels, batch_size, funcs,
                  counts_host=None):
    """core.py:11-46.  instance_logits [R, num_classes]; batch_inds [R] or [R,1] bag index
    of every instance (0-based, grouped and ascending); bag_labels [batch_size] int.
    funcs[0] is used for bags labelled 1, funcs[1] otherwise (:40-42).
    Returns (bag_logits [batch_size, num_classes], scale_factors [batch_size]).
    `counts_host` (instances per bag) avoids a device->host copy when the caller knows it."""
    if counts_host is None:
        b = batch_inds.reshape(-1).to(torch.int64)
        counts_host = torch.bincount(b, minlength=batch_size)[:batch_size].cpu().tolist()
    labels_host = bag_labels.reshape(-1).cpu().tolist() if isinstance(bag_labels, torch.Tensor) \
        else [int(x) for x in bag_labels]
    rows, scales = [], []
    start = 0
    for i in range(batch_size):
        n = int(counts_host[i])
        cur = instance_logits[start:start + n]
        start += n
        f = funcs[0] if int(labels_host[i]) == 1 else funcs[1]
        row = f(cur)
        rows.append(row)
        scales.append(torch.softmax(row, dim=1)[0, int(labels_host[i])])
    return torch.cat(rows, dim=0), torch.stack(scales)


# ------------------------------------------------------------------ device op (f1) ---
# function -> enum wssdl_mil_selector (include/wssdl_bus_hip.h)
_SELECTORS = {get_mal_max_logit: 0, get_ben_max_logit: 1, get_mass_max_logit: 2, get_disc_max_logit: 3,
              get_mean_ben_logit: 4}
_MEAN_BEN = _SELECTORS[get_mean_ben_logit]

# the names a pair is chosen by (SolverWrapper(mil_funcs=...), --mil_funcs)
MIL_FUNCS = {'mal_max': get_mal_max_logit, 'ben_max': get_ben_max_logit, 'mass_max': get_mass_max_logit,
             'disc_max': get_disc_max_logit, 'mean_ben': get_mean_ben_logit}


def resolve_funcs(pair):
    """A pair (for bags labelled 1, for the others) of bag functions or of their names in MIL_FUNCS -> list of the
    two functions.  Anything else raises ValueError."""
    if isinstance(pair, str) or not isinstance(pair, (list, tuple)) or len(pair) != 2:
        raise ValueError("mil_funcs: a pair (for bags labelled 1, for the others) is needed, got %r" % (pair,))
    out = []
    for f in pair:
        if isinstance(f, str):
            if f not in MIL_FUNCS:
                raise ValueError("mil_funcs: unknown bag function %r (one of %s)" % (f, ', '.join(MIL_FUNCS)))
            f = MIL_FUNCS[f]
        elif f not in _SELECTORS:
            raise ValueError("mil_funcs: %r is none of the bag functions of mil.core" % (f,))
        out.append(f)
    return out


def parse_funcs(text):
    """'NAME,NAME' of a command line -> the pair of functions (None stays None)"""
    return None if text is None else resolve_funcs([t.strip() for t in text.split(',')])


def _bag_column(bag_column, R):
    """(f32 column, element stride) as the ops take it: a strided 1-d view such as rois[:, 0] is passed as it is"""
    col = bag_column if bag_column.dtype == torch.float32 else bag_column.to(torch.float32)
    stride = col.stride(0) if col.dim() == 1 and R > 1 else 1
    if col.dim() != 1 or (R > 1 and stride < 1):
        col = col.reshape(-1).contiguous()
        stride = 1
    return col, stride


def get_bag_logit_device(instance_logits, bag_column, bag_offset, bag_labels, batch_size, funcs,
                         return_valid=False):
    """get_bag_logit as ONE kernel launch + one gather, with no host round trip: the HIP op
    ``wssdl_mil_select`` picks each bag's instance row, ``index_select`` (differentiable) gathers
    the logit rows.  A pair that holds get_mean_ben_logit also takes the op's per-bag counts and
    forms the pooled rows [0, mean, 0, ...] with torch ops on the device (an f64 index_add, one
    division, one rounding to f32), differentiable like the gather: every row of such a bag gets
    grad[b, 1] / count in column 1.  `bag_column` is the column holding each instance's bag index plus
    `bag_offset` (a strided view such as ``rois[n_valid:, 0]`` is fine).  Returns
    (bag_logits [batch_size, K], scale_factors [batch_size]) like get_bag_logit.

    A bag without instances (a weak image whose proposals were all filtered out) makes the
    reference's tf.arg_max fail on the host.  Here the op reports row -1 for it; the gather then
    uses row 0 and the bag's logits are zeroed, and with `return_valid` the [batch_size] bool
    mask of the non-empty bags is returned as a third value so that the loss can give such a
    bag zero weight -- all without a device->host copy.  No instances at all raises ValueError."""
    from .. import _lib
    logits = instance_logits.contiguous()
    R, K = logits.shape
    if R == 0 and batch_size > 0:
        raise ValueError("get_bag_logit: no instances for %d bag(s)" % batch_size)
    col, stride = _bag_column(bag_column, R)
    labels = bag_labels.reshape(-1).to(torch.int32).contiguous()
    rows = torch.empty((batch_size,), dtype=torch.int32, device=logits.device)
    sel = (_SELECTORS[funcs[0]], _SELECTORS[funcs[1]])
    pools = _MEAN_BEN in sel
    counts = torch.empty((batch_size,), dtype=torch.int32, device=logits.device) if pools else None
    with torch.cuda.device(logits.device):
        _lib.check(_lib.lib().wssdl_mil_select(
            _lib.ptr(logits), R, K, _lib.ptr(col), int(stride), float(bag_offset), _lib.ptr(labels),
            int(batch_size), sel[0], sel[1], _lib.ptr(rows), _lib.ptr(counts) if pools else None,
            _lib.stream()), "wssdl_mil_select")
    valid = rows >= 0
    bag_logits = instance_logits.index_select(0, rows.clamp_min(0).to(torch.int64))
    if pools:
        # a mean-ben bag: [0, mean of its rows' class-1 logits, 0, ...], the sum in f64 and the mean rounded to f32
        # once like the fused op's; differentiable through index_add (every row of the bag gets grad / count)
        bag = (col - float(bag_offset)).to(torch.int64)            # the op's own f32 subtraction and truncation
        inside = (bag >= 0) & (bag < batch_size)
        x1 = torch.where(inside, instance_logits[:, 1].double(), instance_logits.new_zeros((), dtype=torch.float64))
        sums = torch.zeros((batch_size,), dtype=torch.float64, device=logits.device)
        sums = sums.index_add(0, bag.clamp(0, batch_size - 1), x1)
        mean = (sums / counts.clamp_min(1).double()).to(bag_logits.dtype)
        e1 = torch.zeros((1, K), dtype=bag_logits.dtype, device=logits.device)
        e1[:, 1].fill_(1.0)                                         # (e1[0, 1] = 1.0 uploads a scalar: a host synchronisation)
        pooled = torch.ones_like(valid) if sel[0] == sel[1] else ((labels == 1) if sel[0] == _MEAN_BEN else (labels != 1))
        bag_logits = torch.where(pooled.unsqueeze(1), mean.unsqueeze(1) * e1, bag_logits)
    bag_logits = bag_logits * valid.unsqueeze(1).to(bag_logits.dtype)
    scale = torch.softmax(bag_logits, dim=1).gather(1, labels.to(torch.int64).unsqueeze(1)).squeeze(1)
    if return_valid:
        return bag_logits, scale, valid
    return bag_logits, scale


class _MilLoss(torch.autograd.Function):
    """The MIL term as one device op (csrc/mil.hip): bag function + weighted CE + mean, and its backward.  A selecting
    pair goes through wssdl_mil_loss_forward / _backward as it always has; a pair with mean-ben through
    wssdl_mil_pool_forward / _backward: the same kernels, with the per-bag count and the bags' logit rows kept for the
    backward."""

    @staticmethod
    def forward(ctx, instance_logits, bag_column, bag_offset, bag_labels, n_bags, sel1, sel_other, class_weights, scale):
        import numpy as np
        from .. import _lib
        logits = instance_logits.contiguous()
        R, K = logits.shape
        col, stride = _bag_column(bag_column, R)
        labels = bag_labels.reshape(-1).to(torch.int32).contiguous()
        dev = logits.device
        rows = torch.empty((n_bags,), dtype=torch.int32, device=dev)
        bag_loss = torch.empty((n_bags,), dtype=torch.float32, device=dev)
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        cw = np.ascontiguousarray(np.asarray(class_weights, np.float32))
        pools = sel1 == _MEAN_BEN or sel_other == _MEAN_BEN
        with torch.cuda.device(dev), _lib.timed("mil_loss", dict(R=R, bags=int(n_bags))):
            if pools:
                counts = torch.empty((n_bags,), dtype=torch.int32, device=dev)
                bag_logits = torch.empty((n_bags, K), dtype=torch.float32, device=dev)
                _lib.check(_lib.lib().wssdl_mil_pool_forward(
                    _lib.ptr(logits), R, K, _lib.ptr(col), int(stride), float(bag_offset), _lib.ptr(labels), int(n_bags),
                    int(sel1), int(sel_other), _lib.host_ptr(cw), float(scale), _lib.ptr(loss), _lib.ptr(rows),
                    _lib.ptr(counts), _lib.ptr(bag_logits), _lib.ptr(bag_loss), _lib.stream()), "wssdl_mil_pool_forward")
                ctx.save_for_backward(logits, col, labels, rows, counts, bag_logits)
            else:
                _lib.check(_lib.lib().wssdl_mil_loss_forward(
                    _lib.ptr(logits), R, K, _lib.ptr(col), int(stride), float(bag_offset), _lib.ptr(labels), int(n_bags),
                    int(sel1), int(sel_other), _lib.host_ptr(cw), float(scale), _lib.ptr(loss), _lib.ptr(rows),
                    _lib.ptr(bag_loss), _lib.stream()), "wssdl_mil_loss_forward")
                ctx.save_for_backward(logits, col, labels, rows)
        ctx.misc = (R, K, int(stride), float(bag_offset), int(n_bags), cw, float(scale), int(sel1), int(sel_other), pools)
        return loss[0]

    @staticmethod
    def backward(ctx, grad_loss):
        from .. import _lib
        saved = ctx.saved_tensors
        logits = saved[0]
        R, K, stride, bag_offset, n_bags, cw, scale, sel1, sel_other, pools = ctx.misc
        g = torch.empty_like(logits)
        gl = grad_loss.reshape(1).to(torch.float32).contiguous()
        with torch.cuda.device(logits.device), _lib.timed("mil_loss_backward", dict(R=R, bags=n_bags)):
            if pools:
                logits, col, labels, rows, counts, bag_logits = saved
                _lib.check(_lib.lib().wssdl_mil_pool_backward(
                    _lib.ptr(logits), R, K, _lib.ptr(col), stride, bag_offset, _lib.ptr(labels), n_bags, sel1, sel_other,
                    _lib.ptr(rows), _lib.ptr(counts), _lib.ptr(bag_logits), _lib.host_ptr(cw), scale, _lib.ptr(gl),
                    _lib.ptr(g), _lib.stream()), "wssdl_mil_pool_backward")
            else:
                logits, col, labels, rows = saved
                _lib.check(_lib.lib().wssdl_mil_loss_backward(
                    _lib.ptr(logits), R, K, _lib.ptr(col), stride, bag_offset, _lib.ptr(labels), n_bags, _lib.ptr(rows),
                    _lib.host_ptr(cw), scale, _lib.ptr(gl), _lib.ptr(g), _lib.stream()), "wssdl_mil_loss_backward")
        return (g,) + (None,) * 8


@torch.no_grad()
def mil_bag_losses_device(instance_logits, bag_column, bag_offset, bag_labels, n_bags, funcs, class_weights):
    """[n_bags] f32: class_weights[label] * CE(the bag's logit row, label) of every bag, 0 for an empty bag --
    the per-bag output of the fused op (bag_loss of wssdl_mil_loss_forward, or of wssdl_mil_pool_forward when the pair
    holds mean-ben) in one call, forward only.  The op's own loss is mean(bag_loss) * scale; a bag on its own
    (n_bags = 1) has the loss (f32)((f64)scale * bag_loss)."""
    import numpy as np
    from .. import _lib
    if instance_logits.shape[0] == 0 and n_bags > 0:
        raise ValueError("get_bag_logit: no instances for %d bag(s)" % n_bags)
    logits = instance_logits.detach().contiguous()
    R, K = logits.shape
    col, stride = _bag_column(bag_column, R)
    labels = bag_labels.reshape(-1).to(torch.int32).contiguous()
    dev = logits.device
    rows = torch.empty((n_bags,), dtype=torch.int32, device=dev)
    bag_loss = torch.empty((n_bags,), dtype=torch.float32, device=dev)
    loss = torch.empty((1,), dtype=torch.float32, device=dev)
    cw = np.ascontiguousarray(np.asarray(class_weights, np.float32))
    sel1, sel_other = _SELECTORS[funcs[0]], _SELECTORS[funcs[1]]
    with torch.cuda.device(dev), _lib.timed("mil_bag_losses", dict(R=R, bags=int(n_bags))):
        if sel1 == _MEAN_BEN or sel_other == _MEAN_BEN:
            counts = torch.empty((n_bags,), dtype=torch.int32, device=dev)
            bag_logits = torch.empty((n_bags, K), dtype=torch.float32, device=dev)
            _lib.check(_lib.lib().wssdl_mil_pool_forward(
                _lib.ptr(logits), R, K, _lib.ptr(col), int(stride), float(bag_offset), _lib.ptr(labels), int(n_bags),
                sel1, sel_other, _lib.host_ptr(cw), 1.0, _lib.ptr(loss), _lib.ptr(rows), _lib.ptr(counts),
                _lib.ptr(bag_logits), _lib.ptr(bag_loss), _lib.stream()), "wssdl_mil_pool_forward")
        else:
            _lib.check(_lib.lib().wssdl_mil_loss_forward(
                _lib.ptr(logits), R, K, _lib.ptr(col), int(stride), float(bag_offset), _lib.ptr(labels), int(n_bags),
                sel1, sel_other, _lib.host_ptr(cw), 1.0, _lib.ptr(loss), _lib.ptr(rows),
                _lib.ptr(bag_loss), _lib.stream()), "wssdl_mil_loss_forward")
    return bag_loss


def mil_loss_device(instance_logits, bag_column, bag_offset, bag_labels, n_bags, funcs, class_weights, scale):
    """train_bus.py:239-260 / :650-671 on the device: mean over the bags of
    scale * class_weights[label] * CE(the bag's logit row under its bag function, label); an empty bag contributes 0.
    Any pair of the five bag functions.  No instances at all raises ValueError like get_bag_logit_device."""
    if instance_logits.shape[0] == 0 and n_bags > 0:
        raise ValueError("get_bag_logit: no instances for %d bag(s)" % n_bags)
    return _MilLoss.apply(instance_logits, bag_column, bag_offset, bag_labels, int(n_bags), _SELECTORS[funcs[0]],
                          _SELECTORS[funcs[1]], class_weights, scale)
