"""Shared by test_network_reference_cpu.py and test_gpu_network_reference.py: a plain functional statement of the
ResNet trunk (conv0 ... group2/relu) and of the per-RoI head (group3 ... gap), written from the reference project's
wiring and importing nothing from wssdl_bus_amd.networks.  The suites of networks/roi_head.py and
networks/backbones.py above single-layer level compare one route of those files with another; the wiring both routes
share (which tensor a shortcut takes, which norm follows a block, the slot order and the final mean, which buffers
are updated with which n, eps and momentum, where the live-row mask is honoured) is held to this module instead.

THE REFERENCE.  `trunk` / `head` take a state_dict, an input and an upstream gradient and return every output:
'y', 'dx', 'g.<parameter>' and 'b.<buffer>'.  They are dtype- and device-agnostic: the state is cast to the input's
dtype, so the same function is the f64 reference D and, in f32, the stock-ops evaluation S.

  wiring      code/lib/networks/network.py:424-457 (basicblock / bottleneck): 'both_preact' normalises and rectifies the
              input and the shortcut takes THAT tensor; any other preact but 'no_preact' ('default') hands the shortcut
              the RAW input and normalises only the residual branch; 'no_preact' does nothing before conv1.
              :418-422 (shortcut): a 1x1 convolution at the block's stride with norm and no ReLU when the channel
              counts differ, else the identity.  :460-468 (layer_group): block0 'no_preact' if first else
              'both_preact' at the group's stride, then count-1 'default' blocks at stride 1.
              Resnet_train_bus.py:30-35 (depth table), :55-63 (trunk: conv0 7x7/2 with norm and ReLU, 3x3/2 'VALID'
              max pool, group0 (first, 64, stride 1), group1 (128, stride 2), group2 (256, stride 2), norm, ReLU),
              :91-97 (head: group3 (512, stride 2), norm, ReLU, mean over the positions).
  convolution an explicit sum over taps on NHWC tensors: TF-'SAME' padding (asymmetric, the odd unit AFTER), then
              for each (kh, kw) one matmul of the strided slice with that tap's [c_i, c_o] weight.  No unfold, no
              conv2d, no tap plan, no library convolution.  The head's ConvNHWC.weight is [c_o, k*k*c_i] with the
              patch laid out (kh, kw, c_i); the trunk's nn.Conv2d weight is OIHW.  There is no bias next to a norm.
  batch norm  mean and biased variance over all rows, eps 1e-3, in plain tensor ops; running statistics
              r <- r + 0.01 * (batch - r) with the variance unbiased by n / (n - 1); the trunk's
              num_batches_tracked advances by 1.  In eval mode the running buffers are used and left alone.
  gradients   autograd on this function, loss = sum(y * dy).
  live rows   there is no mask here: `live` (indices of the live RoIs) compacts input and upstream gradient first, n
              is the live row count, and 'y' / 'dx' are returned for the live RoIs only.

`defect=` seeds one wiring mistake (DEFECTS) and exists for test_network_reference_cpu.py, which shows that the
criterion below sees each of them.

THE CRITERION.  A composite network has no countable elementwise bound, so the yardstick is the reference itself in
f32.  For every output tensor, norms in f64:

    err(H) = ||H - D||_2
    floor  = max(||S - D||_2, 2^-24 * ||D||_2, 2^-24 * ||D_sib||_2)
    err(H) <= K * floor

H the route under test, D and S this module in f64 / f32 on the same device, D_sib (bias gradients of norms only) the
f64 weight gradient of the same norm: the bias gradient of a norm whose output reaches nothing but a training-mode
batch norm (through the residual adds) is zero in exact arithmetic -- the next norm removes per-channel shifts -- so D
is ~1e-17 there and only the scale of the sums that produced it means anything; the sibling gradient is that scale.
`ratios` computes err / floor for every tensor, `check_nonzero` holds ||D|| > 0 for y, dx and every weight gradient,
`output_class` names the seven classes the worst ratios are reported by.
"""
import torch
import torch.nn.functional as F

# Resnet_train_bus.py:30-35
DEPTHS = {18: ([2, 2, 2, 2], "basic"), 34: ([3, 4, 6, 3], "basic"),
          50: ([3, 4, 6, 3], "bottleneck"), 101: ([3, 4, 23, 3], "bottleneck")}
EPS, MOMENTUM = 1e-3, 0.01

DEFECTS = {
    "a": "both_preact shortcut fed the raw input",
    "b": "default shortcut fed the pre-activation",
    "c": "eps 1e-5",
    "d": "'SAME' padding before-heavy",
    "e": "running variance without the unbiasing",
    "f": "head mean over 49 positions' worth of rows instead of the 16 slots",
    "g": "statistics over all rows, dead ones included",
}

CLASSES = ("y", "dx", "conv weight grad", "norm weight grad", "norm bias grad", "running mean", "running var")
U32 = 2.0 ** -24


class _Net:
    """One evaluation: the parameters as autograd leaves of the input's dtype, the new buffer values as they come."""

    def __init__(self, state, like, training, defect):
        assert defect is None or defect in DEFECTS, defect
        self.training, self.defect = training, defect
        self.buffers = {k for k in state if k.rsplit(".", 1)[-1] in ("running_mean", "running_var",
                                                                    "num_batches_tracked")}
        self.p, self.b = {}, {}
        for k, v in state.items():
            v = v.detach().to(like.device)
            if k in self.buffers:
                self.b[k] = v.to(like.dtype) if v.dtype.is_floating_point else v.clone()
            else:
                self.p[k] = v.to(like.dtype).clone().requires_grad_(True)
        self.used = set()

    def param(self, key):
        self.used.add(key)
        return self.p[key]

    # ---- layers ----
    def same_pad(self, size, k, s):
        out = -(-size // s)
        total = max((out - 1) * s + k - size, 0)
        before = total // 2
        if self.defect == "d":
            before = total - before
        return before, total - before

    def conv(self, x, key, k, s, layout, padding="SAME"):
        """x [N, H, W, c_i] -> [N, oh, ow, c_o]: the sum over the k*k taps."""
        w = self.param(key)
        c_i = x.shape[3]
        if layout == "rows":                                  # [c_o, (kh, kw, c_i)]
            taps = w.view(w.shape[0], k, k, c_i).permute(1, 2, 3, 0)
        else:                                                 # OIHW
            assert w.shape[1:] == (c_i, k, k)
            taps = w.permute(2, 3, 1, 0)
        if padding == "SAME":
            pt, pb = self.same_pad(x.shape[1], k, s)
            pl, pr = self.same_pad(x.shape[2], k, s)
            x = F.pad(x, (0, 0, pl, pr, pt, pb))
        oh, ow = (x.shape[1] - k) // s + 1, (x.shape[2] - k) // s + 1
        y = None
        for kh in range(k):
            for kw in range(k):
                t = torch.matmul(x[:, kh:kh + (oh - 1) * s + 1:s, kw:kw + (ow - 1) * s + 1:s, :], taps[kh, kw])
                y = t if y is None else y + t
        return y

    def norm(self, x, prefix, relu):
        """Batch norm over all leading axes of [..., C]."""
        w, b = self.param(prefix + ".weight"), self.param(prefix + ".bias")
        eps = 1e-5 if self.defect == "c" else EPS
        rm, rv = prefix + ".running_mean", prefix + ".running_var"
        self.used.update((rm, rv))
        if self.training:
            rows = x.reshape(-1, x.shape[-1])
            n = rows.shape[0]
            mean = rows.mean(0)
            var = ((rows - mean) ** 2).mean(0)
            with torch.no_grad():
                unbias = 1.0 if self.defect == "e" else n / max(n - 1, 1)
                self.b[rm] = self.b[rm] + MOMENTUM * (mean - self.b[rm])
                self.b[rv] = self.b[rv] + MOMENTUM * (var * unbias - self.b[rv])
                nbt = prefix + ".num_batches_tracked"
                if nbt in self.b:
                    self.b[nbt] = self.b[nbt] + 1
        else:
            mean, var = self.b[rm], self.b[rv]
        y = (x - mean) / torch.sqrt(var + eps) * w + b
        return torch.relu(y) if relu else y

    def conv_int(self, x, prefix, k, s, layout, relu=True):
        """network.py conv_int: convolution, norm, optional ReLU."""
        key = prefix + (".weight" if layout == "rows" else ".conv.weight")
        return self.norm(self.conv(x, key, k, s, layout), prefix + ".bn", relu)

    def block(self, x, prefix, kind, c_o, s, preact, layout):
        """network.py:424-457."""
        c_i = x.shape[3]
        if preact == "both_preact":
            raw = x
            x = self.norm(x, prefix + ".pre_bn", True)
            ori = raw if self.defect == "a" else x
        elif preact != "no_preact":
            ori = x
            x = self.norm(x, prefix + ".pre_bn", True)
            if self.defect == "b":
                ori = x
        else:
            ori = x
        if kind == "basic":
            x = self.conv_int(x, prefix + ".conv1", 3, s, layout)
            x = self.conv_int(x, prefix + ".conv2", 3, 1, layout, relu=False)
            c_out = c_o
        else:
            x = self.conv_int(x, prefix + ".conv1", 1, 1, layout)
            x = self.conv_int(x, prefix + ".conv2", 3, s, layout)
            x = self.conv_int(x, prefix + ".conv3", 1, 1, layout, relu=False)
            c_out = c_o * 4
        if c_i != c_out:                                      # network.py:418-422
            ori = self.conv_int(ori, prefix + ".short", 1, s, layout, relu=False)
        return x + ori

    def group(self, x, name, kind, c_o, count, s, layout, first=False):
        """network.py:460-468."""
        x = self.block(x, name + ".0", kind, c_o, s, "no_preact" if first else "both_preact", layout)
        for i in range(1, count):
            x = self.block(x, "%s.%d" % (name, i), kind, c_o, 1, "default", layout)
        return x

    def outputs(self, y, x, dy, permute=None):
        assert self.used == set(self.p) | {k for k in self.b if not k.endswith("num_batches_tracked")}, \
            sorted((set(self.p) | set(self.b)) ^ self.used)
        out = {}
        leaves = [x] + list(self.p.values())
        grads = torch.autograd.grad((y * dy).sum(), leaves)
        out["y"], out["dx"] = y.detach(), grads[0]
        if permute is not None:
            out["y"], out["dx"] = out["y"].permute(*permute), out["dx"].permute(*permute)
        for k, g in zip(self.p, grads[1:]):
            out["g." + k] = g
        for k, v in self.b.items():
            out["b." + k] = v
        return out


def _max_pool_3x3_s2_valid(x):
    oh, ow = (x.shape[1] - 3) // 2 + 1, (x.shape[2] - 3) // 2 + 1
    y = None
    for kh in range(3):
        for kw in range(3):
            t = x[:, kh:kh + (oh - 1) * 2 + 1:2, kw:kw + (ow - 1) * 2 + 1:2, :]
            y = t if y is None else torch.maximum(y, t)       # ties are between rectified zeros: no gradient there
    return y


def trunk(state, x, dy, depth, training=True, defect=None):
    """Resnet_train_bus.py:55-63.  state: ResNetTrunk(depth).state_dict(); x [N, 3, H, W], dy the gradient of the
    [N, C, h, w] output (any memory format; values only).  Returns the dict of outputs in x's dtype."""
    defs, kind = DEPTHS[depth]
    e = 4 if kind == "bottleneck" else 1
    net = _Net(state, x, training, defect)
    xin = x.detach().permute(0, 2, 3, 1).contiguous().requires_grad_(True)
    h = net.conv_int(xin, "conv0", 7, 2, "oihw")
    h = _max_pool_3x3_s2_valid(h)
    h = net.group(h, "group0", kind, 64, defs[0], 1, "oihw", first=True)
    h = net.group(h, "group1", kind, 128, defs[1], 2, "oihw")
    h = net.group(h, "group2", kind, 256, defs[2], 2, "oihw")
    h = net.norm(h, "norm", True)
    assert h.shape[3] == 256 * e
    return net.outputs(h, xin, dy.detach().permute(0, 2, 3, 1).to(x.dtype), permute=(0, 3, 1, 2))


def head(state, x, dy, depth, training=True, defect=None, live=None):
    """Resnet_train_bus.py:91-97.  state: ResNetHeadNHWC(depth).state_dict(); x [R, 7, 7, C] NHWC, dy [R, 512*e].
    live: indices of the live RoIs (the others do not exist for the reference); 'y' and 'dx' are then those of the
    live RoIs, in order."""
    defs, kind = DEPTHS[depth]
    net = _Net(state, x, training, defect)
    x, dy = x.detach(), dy.detach().to(x.dtype)
    if live is not None and defect != "g":
        x, dy = x[live], dy[live]
    elif live is not None:                                    # defect 'g': every row enters every statistic
        keep = torch.zeros(x.shape[0], dtype=x.dtype, device=x.device)
        keep[live] = 1.0
        dy = dy * keep.unsqueeze(1)
    xin = x.clone().requires_grad_(True)
    h = net.group(xin, "group3", kind, 512, defs[3], 2, "rows")
    h = net.norm(h, "norm", True)
    if defect == "f":
        y = h.sum(dim=(1, 2)) / float(xin.shape[1] * xin.shape[2])
    else:
        y = h.mean(dim=(1, 2))
    out = net.outputs(y, xin, dy)
    if live is not None and defect == "g":
        out["y"], out["dx"] = out["y"][live], out["dx"][live]
    return out


# ---- the criterion ----
def is_norm_key(name, keys):
    """True for 'g.<norm>.weight' / 'g.<norm>.bias': the norm is the module that also owns a running_mean."""
    if not name.startswith("g."):
        return False
    mod = name[2:].rsplit(".", 1)[0]
    return "b." + mod + ".running_mean" in keys


def output_class(name, keys):
    if name in ("y", "dx"):
        return name
    if name.startswith("g."):
        if is_norm_key(name, keys):
            return "norm weight grad" if name.endswith(".weight") else "norm bias grad"
        return "conv weight grad"
    if name.endswith("running_mean"):
        return "running mean"
    if name.endswith("running_var"):
        return "running var"
    return None                                              # num_batches_tracked: compared exactly


def _norm(t):
    return float(t.double().norm())


def floor(name, S, D):
    """max(||S - D||, 2^-24 ||D||, 2^-24 ||D_sib||) of one tensor."""
    d = D[name].double()
    f = max(_norm(S[name].double() - d), U32 * _norm(d))
    if name.endswith(".bias") and is_norm_key(name, D.keys()):
        f = max(f, U32 * _norm(D[name[:-len("bias")] + "weight"]))
    return f


def ratios(H, S, D):
    """err(H) / floor for every floating-point tensor of D; H must hold the same tensors."""
    assert set(H) == set(D) == set(S), sorted(set(H) ^ set(D))
    out = {}
    for name, d in D.items():
        if not d.dtype.is_floating_point:
            continue
        h = H[name]
        assert h.shape == d.shape, (name, tuple(h.shape), tuple(d.shape))
        assert bool(torch.isfinite(h).all()), name
        out[name] = _norm(h.double() - d.double()) / floor(name, S, D)
    return out


def check_nonzero(D):
    """||D|| > 0 for y, dx and every weight gradient: a comparison with a zero reference would say nothing."""
    for name, d in D.items():
        if name in ("y", "dx") or (name.startswith("g.") and name.endswith(".weight")):
            assert _norm(d) > 0.0, name


def worst_by_class(rat, keys):
    """{class: (ratio, tensor name)} of the largest ratio in each output class."""
    worst = {}
    for name, r in rat.items():
        c = output_class(name, keys)
        if c is not None and r >= worst.get(c, (-1.0, ""))[0]:
            worst[c] = (r, name)
    return worst


def module_outputs(module, y, x):
    """The outputs of one forward / backward of an nn.Module in the reference's naming."""
    out = {"y": y.detach(), "dx": x.grad}
    for k, p in module.named_parameters():
        assert p.grad is not None, k
        out["g." + k] = p.grad
    for k, b in module.named_buffers():
        out["b." + k] = b.detach().clone()
    return out


def prepare(module):
    """Non-trivial weights for a freshly built trunk or head (from torch's global generator): convolution weights
    x 20 (activations of order 1 through the depth), norm weights in [0.5, 1.5], biases in [-0.2, 0.2], running
    buffers away from their initial 0 / 1.  Returns the module in training mode."""
    with torch.no_grad():
        for m in module.modules():
            if getattr(m, "running_mean", None) is not None:
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
                m.running_mean.uniform_(-0.1, 0.1)
                m.running_var.uniform_(0.5, 2.0)
            elif "weight" in m._parameters:
                m.weight.mul_(20.0)
    return module.train()
