"""The reference's optimisers and learning-rate schedules (code/lib/fast_rcnn/train_bus.py:32-94, :274-294, :694-697).

ReferenceOptimizer is what `--opt adam|amsgrad|sgd` selects there, in TensorFlow 1.x's arithmetic:

  adam     tf.train.AdamOptimizer(lr, epsilon=0.1), the "epsilon-hat" form of the paper:
               alpha_t = lr * sqrt(1 - b2^t) / (1 - b1^t)
               m += (g - m) * (1 - b1);  v += (g * g - v) * (1 - b2);  p -= (m * alpha_t) / (sqrt(v) + eps)
           torch.optim.Adam divides by sqrt(v) / sqrt(1 - b2^t) + eps instead: in these terms its epsilon is
           eps * sqrt(1 - b2^t), 0.0032 at t = 1 where TF's is 0.1.  With eps = 0.1 above most gradients the two
           differ by the factor 30 at the first step (tests/test_optim_cpu.py states the figure).
  amsgrad  Adam's m and v, then vhat = max(vhat, v) and p -= (m * alpha_t) / (sqrt(vhat) + eps).  The reference's
           AMSGrad module is not in its tree (its import is commented out, train_bus.py:28), so this is the published
           algorithm in TF Adam's epsilon-hat form: parity with whatever the authors ran is UNPINNED.
  sgd      tf.train.MomentumOptimizer(lr, cfg.TRAIN.MOMENTUM, use_nesterov=True), the ApplyMomentum kernel:
               accum = accum * mu + g;  p -= g * lr + (accum * mu) * lr

All of it f32, every operation rounded on its own in the order written.  alpha_t is computed here in f64 from this
object's own step count and rounded to f32 once.  Two routes compute the same formulas:

* one HIP launch over every parameter (csrc/plumbing/optim.hip), when every parameter is a dense f32 tensor on one GPU
  and the plumbing library is loaded (hip_usable);
* otherwise, or with WSSDL_TORCH_OPTIM set, a per-parameter chain of torch ops in the same operation order (about
  ten launches per parameter on a GPU; also what CPU tensors take).

The state (m, v, vhat / accum) lives in flat f32 buffers owned by the optimiser, every parameter starting on a float4
and laid out in its own storage order; state_dict() hands out per-parameter views of them.

ReduceLROnPlateau and piecewise_lr are the `--lr_scheduling rop|pc` schedules, host arithmetic only.
"""
import math

import numpy as np
import torch

from ..networks import _plumbing
from ..networks._plumbing import _p, _call, _storage_dense

CHUNK = 4096                        # floats per chunk: keep in sync with CHUNK of optim.hip
ALIGN = 4                           # every parameter starts on a float4 of the flat state buffers
KINDS = {"adam": 0, "amsgrad": 1, "sgd": 2}
SLOTS = {"adam": ("m", "v"), "amsgrad": ("m", "v", "vhat"), "sgd": ("accum",)}
TABLE_BUILDS = [0]                  # chunk tables built so far (tests read it)


def _f32(x):
    """x rounded to f32, as a Python float (what a kernel argument passed by value holds)"""
    return float(np.float32(x))


def adam_alpha(lr, b1, b2, t):
    """alpha_t = lr * sqrt(1 - b2^t) / (1 - b1^t) in f64, rounded to f32 once"""
    return _f32(float(lr) * math.sqrt(1.0 - float(b2) ** t) / (1.0 - float(b1) ** t))


def _static_usable(params):
    """every parameter a dense f32 tensor on the same GPU"""
    dev = params[0].device
    return all(p.is_cuda and p.device == dev and p.dtype == torch.float32 and _storage_dense(p) for p in params)


def hip_usable(params):
    """True when the one-launch kernel takes this parameter list: every one a dense f32 tensor on the same GPU."""
    if _plumbing.switch("WSSDL_TORCH_OPTIM") or not params:
        return False
    return _static_usable(params) and _plumbing.lib() is not None


class _Table:
    """Device tables of optim.hip for one parameter list.  `chunks`: row i = (parameter index, first float of chunk i
    inside that parameter's storage, its length, its element offset in the flat state buffers), the parameters
    walked in storage order; `params`: the parameters' addresses.
    Built once per parameter list, with two blocking copies from the host that synchronise it; a step has none."""

    def __init__(self, params, offsets):
        rows = []
        for i, (p, off) in enumerate(zip(params, offsets)):
            n = p.numel()
            for first in range(0, n, CHUNK):
                rows.append((i, first, min(CHUNK, n - first), off + first))
        dev = params[0].device
        self.n_chunks = len(rows)
        self.chunks = torch.tensor(rows, dtype=torch.int64).to(dev)
        self.params = torch.tensor([p.data_ptr() for p in params], dtype=torch.int64).to(dev)


class ReferenceOptimizer(object):
    """The part of the torch.optim surface the solver uses -- step(), zero_grad(set_to_none=True),
    param_groups[0]['lr'], state_dict(), load_state_dict() -- over the reference's three optimisers (module
    docstring).  A parameter whose .grad is None is left untouched, state included (apply_gradients with a None
    gradient); the step count still advances, as TF's beta powers do."""

    def __init__(self, params, kind, lr, eps=0.1, betas=(0.9, 0.999), momentum=0.9):
        if kind not in KINDS:
            raise ValueError("unknown optimiser %r (one of %s)" % (kind, ", ".join(sorted(KINDS))))
        self.kind = kind
        self.params = list(params)
        if not self.params:
            raise ValueError("no parameters to optimise")
        self.param_groups = [dict(params=self.params, lr=float(lr))]
        self.eps, self.betas, self.momentum = float(eps), (float(betas[0]), float(betas[1])), float(momentum)
        self.t = 0                                           # steps taken: the t of alpha_t
        self._table = None                                   # (key, _Table)
        self._usable = None                                  # (key, the parameters' part of hip_usable)
        # flat state when every parameter is dense on one device (every layout the networks use); else one tensor
        # per parameter
        dev = self.params[0].device
        self._flat = all(p.device == dev and p.dtype == torch.float32 and _storage_dense(p) for p in self.params)
        self.offsets, off = [], 0
        for p in self.params:
            self.offsets.append(off)
            off += -(-p.numel() // ALIGN) * ALIGN
        if self._flat:
            self.buffers = {s: torch.zeros((off,), dtype=torch.float32, device=dev) for s in SLOTS[kind]}
            # (as_strided's offset counts from the storage's start, not from b's own first element)
            self.views = {s: [b.as_strided(p.shape, p.stride(), b.storage_offset() + o)
                              for p, o in zip(self.params, self.offsets)] for s, b in self.buffers.items()}
        else:
            self.buffers = None
            self.views = {s: [torch.zeros_like(p, memory_format=torch.preserve_format) for p in self.params]
                          for s in SLOTS[kind]}

    # ------------------------------------------------------------------ torch.optim surface
    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if p.grad is None:
                continue
            if set_to_none:
                p.grad = None
            else:
                p.grad.detach_().zero_()

    def state_dict(self):
        """{'kind', 'step', 'lr', 'state': {i: {slot: view of parameter i's state}}}: views, not copies."""
        return dict(kind=self.kind, step=self.t, lr=self.param_groups[0]["lr"],
                    state={i: {s: v[i] for s, v in self.views.items()} for i in range(len(self.params))})

    def load_state_dict(self, sd):
        if sd["kind"] != self.kind or len(sd["state"]) != len(self.params):
            raise ValueError("state of another optimiser: %r, %d parameters" % (sd["kind"], len(sd["state"])))
        with torch.no_grad():
            for i in range(len(self.params)):
                for s, v in self.views.items():
                    src = sd["state"][i][s]
                    if tuple(src.shape) != tuple(v[i].shape):
                        raise ValueError("state %s of parameter %d has shape %s" % (s, i, tuple(src.shape)))
                    v[i].copy_(src)
        self.t = int(sd["step"])
        self.param_groups[0]["lr"] = float(sd["lr"])

    @torch.no_grad()
    def step(self):
        grads = [self._grad_like(p) for p in self.params]    # (raises before anything is changed)
        lr = _f32(self.param_groups[0]["lr"])
        self.t += 1
        b1, b2 = self.betas
        alpha = adam_alpha(lr, b1, b2, self.t) if self.kind != "sgd" else 0.0
        key = tuple((p.data_ptr(), p.shape, p.stride()) for p in self.params)
        if self._usable is None or self._usable[0] != key:   # what hip_usable reads is in the key: checked once per key
            self._usable = (key, _static_usable(self.params))
        if self._usable[1] and not _plumbing.switch("WSSDL_TORCH_OPTIM") and _plumbing.lib() is not None:
            self._step_hip(grads, lr, alpha, key)
        else:
            self._step_torch(grads, lr, alpha)

    # ------------------------------------------------------------------ the two routes
    @staticmethod
    def _grad_like(p):
        """p.grad in p's own layout (the kernel walks both in p's storage order), None when there is none"""
        g = p.grad
        if g is None:
            return None
        if g.dtype != p.dtype or g.device != p.device or g.layout != torch.strided:
            raise ValueError("gradient of a %s parameter is %s, %s on %s" % (tuple(p.shape), g.dtype, g.layout, g.device))
        gs, ps = g.stride(), p.stride()
        if gs != ps and any(a != b for n, a, b in zip(p.shape, gs, ps) if n != 1):       # (size-1 dims: any stride)
            g = torch.empty_strided(p.shape, ps, dtype=p.dtype, device=p.device).copy_(g)
        return g

    def _tables(self, key):
        """The static tables, cached on the parameters' (data_ptr, shape, stride) while they stay where they are (the
        update is in place, so a training run builds them once); a re-allocated parameter rebuilds them."""
        if self._table is None or self._table[0] != key:
            assert _plumbing.lib().wsplumb_optim_chunk() == CHUNK
            self._table = (key, _Table(self.params, self.offsets))
            TABLE_BUILDS[0] += 1
        return self._table[1]

    def _step_hip(self, grads, lr, alpha, key):
        assert self._flat
        tab = self._tables(key)
        dev = self.params[0].device
        # the per-step table: pinned host memory and an asynchronous copy, so no host synchronisation (the pinned
        # block is not reused before the copy has run: the host allocator records the stream)
        addr = torch.tensor([0 if g is None else g.data_ptr() for g in grads], dtype=torch.int64).pin_memory()
        with torch.cuda.device(dev):
            addr = addr.to(dev, non_blocking=True)
        buf = [self.buffers[s] for s in SLOTS[self.kind]] + [None, None]
        b1, b2 = self.betas
        _call("wsplumb_optim_step", dev, KINDS[self.kind], _p(tab.chunks), tab.n_chunks, _p(tab.params), _p(addr),
              len(self.params), _p(buf[0]), _plumbing._pn(buf[1]), _plumbing._pn(buf[2]), lr, alpha, _f32(self.eps),
              _f32(self.momentum), _f32(b1), _f32(b2))

    def _step_torch(self, grads, lr, alpha):
        """the same formulas, one torch op per operation of the kernel (f32 scalars: what the kernel is passed)"""
        one = np.float32(1.0)
        omb1, omb2 = float(one - np.float32(self.betas[0])), float(one - np.float32(self.betas[1]))
        eps, mu = _f32(self.eps), _f32(self.momentum)
        for i, (p, g) in enumerate(zip(self.params, grads)):
            if g is None:
                continue
            if self.kind == "sgd":
                accum = self.views["accum"][i]
                accum.mul_(mu).add_(g)
                p.sub_(g * lr + (accum * mu) * lr)
                continue
            m, v = self.views["m"][i], self.views["v"][i]
            m.add_((g - m) * omb1)
            v.add_((g * g - v) * omb2)
            den = v
            if self.kind == "amsgrad":
                den = self.views["vhat"][i]
                torch.maximum(den, v, out=den)
            p.sub_((m * alpha) / (den.sqrt() + eps))


def make(kind, params, lr):
    """The optimiser `--opt kind` builds in the reference: epsilon 0.1, TF's default betas, cfg.TRAIN.MOMENTUM."""
    from .config import cfg
    return ReferenceOptimizer(params, kind, lr, eps=0.1, betas=(0.9, 0.999), momentum=cfg.TRAIN.MOMENTUM)


# ------------------------------------------------------------------ learning-rate schedules

def piecewise_lr(lr, global_step, max_iters):
    """`--lr_scheduling pc` (train_bus.py:276-279): tf.train.piecewise_constant(global_step, [int(0.75 * max_iters)],
    [lr, 0.1 * lr]).  TF keeps the first value while global_step <= boundary, so the first step taken at the reduced
    rate is the one that starts from global_step = boundary + 1."""
    return lr if int(global_step) <= int(max_iters * 0.75) else lr * 0.1


class ReduceLROnPlateau(object):
    """`--lr_scheduling rop` (train_bus.py:32-94, built at :281 with factor 0.5, patience 5, mode 'min',
    epsilon 1e-3, cooldown 0, min_lr 0): halve the rate when the validation loss has stopped improving.

    After each validation pass on_val_end(loss):
    * during a cool-down the cool-down counter drops by one and `wait` is cleared;
    * a loss better than `best` by more than epsilon becomes `best` and clears `wait`;
    * otherwise, outside a cool-down: if `wait` has reached `patience` and the rate is above min_lr, the rate becomes
      max(rate * factor, min_lr), the cool-down starts and `wait` is cleared -- and then, reduced or not, `wait`
      goes up by one.
    So `wait` is 1, not 0, right after a reduction: the first reduction comes at the (patience + 1)-th loss without
    improvement, every later one `patience` losses after the one before.  At the floor nothing changes and `wait`
    keeps growing.  These quirks are the reference's and are kept."""

    def __init__(self, init_lr, factor=0.5, patience=5, mode="min", epsilon=1e-4, cooldown=0, min_lr=0.0):
        if factor >= 1.0:
            raise ValueError("ReduceLROnPlateau does not support a factor >= 1.0")
        if mode not in ("min", "max"):
            raise ValueError("mode %r is unknown" % (mode,))
        self.cur_lr = init_lr
        self.factor, self.patience, self.mode, self.epsilon = factor, patience, mode, epsilon
        self.cooldown, self.min_lr = cooldown, min_lr
        self.best = math.inf if mode == "min" else -math.inf
        self.cooldown_counter = 0
        self.wait = 0

    def _better(self, loss):
        return loss < self.best - self.epsilon if self.mode == "min" else loss > self.best + self.epsilon

    def on_val_end(self, val_loss):
        """val_loss: the latest validation loss (or the reference's list of all so far: its last entry)"""
        current = val_loss[-1] if isinstance(val_loss, (list, tuple)) else val_loss
        cooling = self.cooldown_counter > 0
        if cooling:
            self.cooldown_counter -= 1
            self.wait = 0
            cooling = self.cooldown_counter > 0
        if self._better(current):
            self.best = current
            self.wait = 0
        elif not cooling:
            if self.wait >= self.patience and self.cur_lr > self.min_lr:
                self.cur_lr = max(self.cur_lr * self.factor, self.min_lr)
                self.cooldown_counter = self.cooldown
                self.wait = 0
            self.wait += 1

    def get_cur_lr(self):
        return self.cur_lr
