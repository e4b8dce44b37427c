"""fp32 torch restatement of the policy/value/ownership tower.  TEST INFRASTRUCTURE ONLY (parity oracle for net.hip and
the CPU baseline's evaluator).  Only tests/, bench.py's cpu_baseline leg and __graft_entry__.smoke() may import it.

Built from the reference's building blocks -- CNNBlock (model.py:317-324), pre-activation ResidualBlock identity branch
(model.py:238-248), tail BN+ReLU (model.py:62,94), value/ownership head (model.py:65-69, :97-102) and policy head
(model.py:73-76, :107-111) -- with the block count and width as parameters, because BASELINE.json's "N-block x
F-filter" nets cannot be expressed by the reference's hard-coded 9+3 layout (model.py:49-61).  `attention=True` inserts
the reference's Self_Attention (model.py:288-315) in the policy head as model.py:72,106 does.
Pinned against the imported reference modules by tests/test_oracle_net.py (golden: tests/golden/net_blocks.npz).
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


class ConvBnRelu(nn.Module):                 # CNNBlock, model.py:317-324
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(cin, cout, 3, 1, 1), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))

    def forward(self, x):
        return self.conv(x)


class PreActBlock(nn.Module):                # ResidualBlock with input_dim == output_dim, model.py:238-248
    def __init__(self, f):
        super().__init__()
        self.batchnormlize_1 = nn.BatchNorm2d(f)
        self.conv_1 = nn.Conv2d(f, f, 3, 1, 1)
        self.batchnormlize_2 = nn.BatchNorm2d(f)
        self.conv_2 = nn.Conv2d(f, f, 3, 1, 1)

    def forward(self, x):
        y = self.conv_1(F.relu(self.batchnormlize_1(x)))
        y = self.conv_2(F.relu(self.batchnormlize_2(y)))
        return x + y


class SelfAttention(nn.Module):              # Self_Attention, model.py:288-315
    def __init__(self, f):
        super().__init__()
        self.query_conv = nn.Conv2d(f, f // 4, 1)
        self.key_conv = nn.Conv2d(f, f // 4, 1)
        self.value_conv = nn.Conv2d(f, f, 1)
        self.gamma = nn.Parameter(torch.zeros(1))
        self.bn = nn.BatchNorm2d(f)

    def forward(self, x):
        b, c, w, h = x.size()
        q = self.query_conv(x).view(b, -1, w * h).permute(0, 2, 1)
        k = self.key_conv(x).view(b, -1, w * h)
        att = torch.softmax(torch.bmm(q, k), dim=-1)
        v = self.value_conv(x).view(b, -1, w * h)
        out = torch.bmm(v, att).view(b, c, w, h)          # sums over the softmaxed row index, as the reference does
        return F.relu(self.bn(self.gamma * out + x))


class TransGoMainBody(nn.Module):
    """MainNetwork (model.py:41-114) with its module names, so the reference state_dict loads unchanged."""

    def __init__(self, board_size, input_dim, f):
        super().__init__()
        self.S = board_size
        P = board_size * board_size
        self.conv1 = ConvBnRelu(input_dim, f)
        for i in range(2, 14):
            setattr(self, f"res_conv{i}", SelfAttention(f) if i in (3, 7, 12) else PreActBlock(f))
        self.bn_res_end = nn.BatchNorm2d(f)
        self.conv_val_own = ConvBnRelu(f, 2)
        self.fc_val_own = nn.Linear(2 * P, 64)
        self.fc_val = nn.Linear(64, 1)
        self.fc_own = nn.Linear(64, P)
        self.attention_act = SelfAttention(f)
        self.conv_act = ConvBnRelu(f, 4)
        self.fc_act = nn.Linear(4 * P, P + 1)

    def forward(self, x):
        P = self.S * self.S
        x = self.conv1(x)
        for i in range(2, 14):
            x = getattr(self, f"res_conv{i}")(x)
        x = F.relu(self.bn_res_end(x))
        h = F.relu(self.fc_val_own(self.conv_val_own(x).view(-1, 2 * P)))
        val = torch.tanh(self.fc_val(h))
        own = torch.tanh(self.fc_own(h))
        act = torch.softmax(self.fc_act(self.conv_act(self.attention_act(x)).view(-1, 4 * P)), -1)
        return act, val, own


class TransGoMain(nn.Module):
    """TransGoNetwork surface (model.py:11-27) around TransGoMainBody."""

    def __init__(self, board_size=9, input_dim=10, filters=128):
        super().__init__()
        self.main_network = TransGoMainBody(board_size, input_dim, filters)

    def main_prediction(self, state):
        return self.main_network(state)


class TowerBody(nn.Module):
    def __init__(self, board_size, input_dim, filters, blocks):
        super().__init__()
        self.S = board_size
        P = board_size * board_size
        self.conv1 = ConvBnRelu(input_dim, filters)
        self.res_blocks = nn.ModuleList([PreActBlock(filters) for _ in range(blocks)])
        self.bn_res_end = nn.BatchNorm2d(filters)
        self.conv_val_own = ConvBnRelu(filters, 2)
        self.fc_val_own = nn.Linear(2 * P, 64)
        self.fc_val = nn.Linear(64, 1)
        self.fc_own = nn.Linear(64, P)
        self.conv_act = ConvBnRelu(filters, 4)
        self.fc_act = nn.Linear(4 * P, P + 1)

    def forward(self, x):
        P = self.S * self.S
        x = self.conv1(x)
        for b in self.res_blocks:
            x = b(x)
        x = F.relu(self.bn_res_end(x))
        h = F.relu(self.fc_val_own(self.conv_val_own(x).view(-1, 2 * P)))
        val = torch.tanh(self.fc_val(h))
        own = torch.tanh(self.fc_own(h))
        act = torch.softmax(self.fc_act(self.conv_act(x).view(-1, 4 * P)), -1)
        return act, val, own


class TowerNetwork(nn.Module):
    """Same surface as TransGoNetwork (model.py:11-27)."""

    def __init__(self, board_size=9, input_dim=10, filters=128, blocks=6):
        super().__init__()
        self.main_network = TowerBody(board_size, input_dim, filters, blocks)

    def main_prediction(self, state):
        return self.main_network(state)

    def get_weights(self):
        return {k: v.cpu() for k, v in self.state_dict().items()}

    def set_weights(self, weights):
        self.load_state_dict(weights)


def seeded_tower(board_size=9, input_dim=10, filters=128, blocks=6, seed=1234):
    """SURVEY.md §8d synthetic weights: torch default init under manual_seed, BN running_mean ~ N(0, 0.1),
    running_var ~ U(0.5, 1.5)."""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    net = TowerNetwork(board_size, input_dim, filters, blocks).eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
                m.weight.copy_(1.0 + 0.1 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
    return net


def _residual_blocks(net):
    """The PreActBlocks of a TowerNetwork or TransGoMain, in trunk order."""
    return [m for m in net.main_network.modules() if isinstance(m, PreActBlock)]


def parity_weights(net, seed, calib=None, res_gain=None, att_logit=2.0, act_gain=1.0, vo_gain=1.0, head_scales=None):
    """Re-initialise `net` (a TowerNetwork or TransGoMain) in place with weights under which every layer visibly moves the outputs,
    for the float64 parity tests: seeded torch's default init leaves the network nearly constant (policy 0.010-0.014, values within
    0.02), so a kernel that dropped a whole input channel still passes a 1e-3 check.  Here conv and linear weights are He-scaled
    (N(0, 2/fan_in)); the second conv of every residual block is scaled by `res_gain` (default 0.5/sqrt(blocks)) so a deep tower
    does not saturate tanh; BatchNorm is non-trivial (gamma 1+0.2N, beta 0.2N, running mean 0.2N, running var U(0.5, 2)); attention
    has gamma U(0.5, 1) and q/k scaled so the pre-softmax scores of a row spread by about `att_logit` (std: peaked rows, the
    largest weight of a row ~e^5 times the mean; sharper ones make the f32 forward itself ill-conditioned); the dense heads are scaled
    by act_gain (policy) and vo_gain (value, ownership) -- or, given calibration positions `calib`, rescaled on them so that
    the smallest per-row policy logit spread is 2 (at most 14 for the widest row) and the largest |pre-tanh| of value and
    ownership is 2: how far the trunk's scale drifts depends on depth, width and seed.  The two factors of that rescaling come out
    of an f32 forward, whose last bits differ between machines and thread counts; they are left in net.head_scales, and
    `head_scales` applies a pair measured elsewhere instead -- everything else is elementwise arithmetic on the seeded generator's
    numbers, so the weights are then the same bits everywhere.  The properties the tests rely on are asserted by the tests, not
    assumed here.  Returns `net`."""
    g = torch.Generator().manual_seed(seed)
    body = net.main_network
    blocks = _residual_blocks(net)
    if res_gain is None:
        res_gain = 0.5 / max(1, len(blocks)) ** 0.5
    rn = lambda t: torch.randn(t.shape, generator=g, dtype=torch.float64).to(t.dtype)

    def he(m, gain=1.0):
        fan_in = m.weight[0].numel()
        m.weight.copy_(rn(m.weight) * (gain * (2.0 / fan_in) ** 0.5))
        m.bias.copy_(rn(m.bias) * 0.05)

    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                he(m)
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(1.0 + 0.2 * rn(m.weight))
                m.bias.copy_(0.2 * rn(m.bias))
                m.running_mean.copy_(0.2 * rn(m.running_mean))
                m.running_var.copy_(0.5 + 1.5 * torch.rand(m.running_var.shape, generator=g, dtype=torch.float64).float())
        for b in blocks:
            b.conv_2.weight.mul_(res_gain)
            b.conv_2.bias.mul_(res_gain)
        for m in net.modules():
            if isinstance(m, SelfAttention):
                m.gamma.copy_(0.5 + 0.5 * torch.rand(1, generator=g, dtype=torch.float64).float())
                d = m.query_conv.weight.shape[0]
                # q.k sums d products of two ~N(0, 2)-ish terms: scale both so its spread is about att_logit
                s = (att_logit / (2.0 * d ** 0.5)) ** 0.5
                m.query_conv.weight.mul_(s); m.key_conv.weight.mul_(s)
        body.fc_val.weight.mul_(vo_gain); body.fc_own.weight.mul_(vo_gain)
        body.fc_act.weight.mul_(act_gain)
        if calib is not None and head_scales is None:
            out = {}
            hs = [getattr(body, k).register_forward_hook(lambda m, i, o, k=k: out.__setitem__(k, o - m.bias)) for k in ("fc_act", "fc_val", "fc_own")]
            net.main_prediction(torch.as_tensor(calib, dtype=torch.float32))
            for h in hs:
                h.remove()
            spread = out["fc_act"].max(1).values - out["fc_act"].min(1).values
            head_scales = (min(2.0 / float(spread.min()), 14.0 / float(spread.max())),
                           2.0 / max(float(out["fc_val"].abs().max()), float(out["fc_own"].abs().max())))
        if head_scales is not None:
            act, vo = head_scales
            body.fc_act.weight.mul_(act)
            body.fc_val.weight.mul_(vo); body.fc_own.weight.mul_(vo)
            net.head_scales = (act, vo)
    return net


def parity_tower(board_size=9, input_dim=10, filters=128, blocks=6, seed=1234, calib=None, head_scales=None):
    """TowerNetwork with parity_weights (see there), head scales calibrated on the positions `calib` or given as `head_scales`."""
    return parity_weights(TowerNetwork(board_size, input_dim, filters, blocks).eval(), seed, calib, head_scales=head_scales)


def parity_transgo(board_size=9, input_dim=10, filters=128, seed=1234, calib=None, head_scales=None):
    """The shipped MainNetwork layout (TransGoMain, attention included) with parity_weights."""
    return parity_weights(TransGoMain(board_size, input_dim, filters).eval(), seed, calib, head_scales=head_scales)


def float64_forward(net, x, block_hook=None):
    """The same modules evaluated in float64 on the positions `x` (each position's outputs depend on that position only, so `x`
    may be any subset of a batch).  block_hook(i, y) -> y, if given, edits the output of the i-th residual block (mutation tests).
    Returns (policy, value, own) as float64 NumPy arrays."""
    import copy
    m = copy.deepcopy(net).double().eval()
    handles = []
    if block_hook is not None:
        for i, b in enumerate(_residual_blocks(m)):
            handles.append(b.register_forward_hook(lambda mod, inp, out, i=i: block_hook(i, out)))
    with torch.no_grad():
        out = m.main_prediction(torch.as_tensor(x).double())
    for h in handles:
        h.remove()
    return tuple(t.numpy() for t in out)


def half_storage_forward(net, x, half_residual=False, f64=False, block_hook=None):
    """What an fp16-storage / f32-accumulate evaluation of `net` (a TowerNetwork) computes, with the rounding points of the
    HIP fp16 chain (BASELINE config 5): every convolution (stem, tower, the two head convs) takes fp16 weights (BatchNorm
    folded in f64, stored as f32, then rounded to nearest even) and fp16 inputs, products accumulate in f32; the residual
    stream and the dense heads stay f32.  Conv inputs: the 0/1 planes (exact), relu(bn1(x)) and relu(bn2(conv1(.))) inside a
    PreActBlock, relu(bn_res_end(x)) for the head convs.  Only the accumulation order inside a convolution is left free.
    half_residual=True emulates net_precision 2: the residual stream is stored as fp16 as well -- a block's f32 result v feeds the
    next activation unrounded, is rounded once into the stream, and the next block adds its convolution to that rounded value.
    f64=True keeps the same fp16 rounding points (and the f32 storage of the folded weights and biases) but accumulates and carries
    everything else in float64, dense heads included: the reference of the float64 parity tests.  x may then be any subset of a
    batch; block_hook(i, y) -> y edits the output of residual block i (mutation tests)."""
    body = net.main_network
    P = body.S * body.S
    dt = torch.float64 if f64 else torch.float32
    q = lambda t: t.half().to(dt)
    x = torch.as_tensor(x).to(dt)
    dense = lambda lin, t: F.linear(t, lin.weight.to(dt), lin.bias.to(dt))

    def fold(bn):
        s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        return s, bn.bias.double() - bn.running_mean.double() * s

    def conv_bn_relu(block, inp):                      # ConvBnRelu with its BN folded into the fp16 weights
        conv, bn = block.conv[0], block.conv[1]
        s, t = fold(bn)
        w = (conv.weight.double() * s[:, None, None, None]).float()
        b = (conv.bias.double() * s + t).float()
        return F.relu(F.conv2d(inp, q(w), b.to(dt), 1, 1))

    with torch.no_grad():
        y = conv_bn_relu(body.conv1, x)
        res = q(y) if half_residual else y                 # what the next block reads back as its residual
        for i, b in enumerate(body.res_blocks):
            s1, t1 = fold(b.batchnormlize_1)
            s2, t2 = fold(b.batchnormlize_2)
            w1 = (b.conv_1.weight.double() * s2[:, None, None, None]).float()
            b1 = (b.conv_1.bias.double() * s2 + t2).float()
            a = q(F.relu(y * s1.float().to(dt)[None, :, None, None] + t1.float().to(dt)[None, :, None, None]))
            h = q(F.relu(F.conv2d(a, q(w1), b1.to(dt), 1, 1)))
            y = F.conv2d(h, q(b.conv_2.weight), b.conv_2.bias.to(dt), 1, 1) + res
            if block_hook is not None:
                y = block_hook(i, y)
            res = q(y) if half_residual else y
        se, te = fold(body.bn_res_end)
        z = q(F.relu(y * se.float().to(dt)[None, :, None, None] + te.float().to(dt)[None, :, None, None]))
        hid = F.relu(dense(body.fc_val_own, conv_bn_relu(body.conv_val_own, z).view(-1, 2 * P)))
        val = torch.tanh(dense(body.fc_val, hid))
        own = torch.tanh(dense(body.fc_own, hid))
        act = torch.softmax(dense(body.fc_act, conv_bn_relu(body.conv_act, z).view(-1, 4 * P)), -1)
    return act, val, own


# ---- float64 parity comparator -----------------------------------------------------------------------------------------------
# Outputs are compared where an error is not squashed: policy as row-centred log p (softmax is invariant to a shift of the row, so
# this is the logit vector up to that shift), value and ownership as atanh of the output (the pre-tanh value).  One tolerance per
# precision class, set from measured GPU runs (tests/test_gpu_net_parity.py lists the figures): "f32" = exact f32 and f32x3 against
# float64_forward, "f16" = f16 and f16r against half_storage_forward(..., f64=True).
PARITY_TOL = {"f32": 5e-5, "f16": 2e-3}


def logit_space(p, v, o):
    lp = np.log(np.asarray(p, np.float64))
    return lp - lp.mean(1, keepdims=True), np.arctanh(np.asarray(v, np.float64)), np.arctanh(np.asarray(o, np.float64))


def parity_error(got, ref):
    """Largest absolute difference in logit space between two (policy, value, own) triples: (max, [policy, value, own])."""
    e = [float(np.max(np.abs(a - b))) for a, b in zip(logit_space(*got), logit_space(*ref))]
    return max(e), e


def weight_properties(ref):
    """What the parity tests rely on, measured on a reference (policy, value, own): the smallest per-row policy logit spread, the
    smallest probability and the largest |pre-tanh| of value and ownership."""
    lp, zv, zo = logit_space(*ref)
    return {"min_logit_spread": float((lp.max(1) - lp.min(1)).min()), "min_prob": float(np.min(ref[0])),
            "max_pre_tanh": float(max(np.abs(zv).max(), np.abs(zo).max()))}


def check_weight_properties(ref):
    w = weight_properties(ref)
    assert w["min_logit_spread"] >= 1.0, w
    assert w["min_prob"] >= 1e-7, w
    assert w["max_pre_tanh"] <= 3.0, w
    return w


class Mutation:
    """A deliberate bug of the kind a kernel could have, applied to the reference: `edit(net)` changes a copy of the weights (the
    copy can be loaded into the HIP network too), `hook(i, y) -> y` edits the output of residual block i."""

    def __init__(self, name, edit=None, hook=None):
        self.name, self.edit, self.hook = name, edit, hook

    def apply(self, net):
        import copy
        m = copy.deepcopy(net)
        if self.edit is not None:
            with torch.no_grad():
                self.edit(m)
        return m


def _stats(net, x, module, live=None):
    """Mean |input| per channel that `module` sees on the positions x (float32 forward), and the fraction of positions where
    `live`'s output (the activation behind the module, if any) is positive per channel: picks weights on a live path."""
    got = {}
    hs = [module.register_forward_hook(lambda m, i, o: got.__setitem__("in", i[0].detach().abs().mean((0, 2, 3))))]
    if live is not None:
        hs.append(live.register_forward_hook(lambda m, i, o: got.__setitem__("live", (o.detach() > 0).double().mean((0, 2, 3)))))
    with torch.no_grad():
        net.main_prediction(torch.as_tensor(x, dtype=torch.float32))
    for h in hs:
        h.remove()
    return got["in"], got.get("live")


def _pick(w, stats, whole_slice=False):
    """Index (cout, cin[, ky, kx]) of the weight element -- or 3x3 slice -- with the largest |w| x mean |input| (x the live
    fraction of its output channel): zeroing it changes the outputs the most, where an element on a dead channel would change
    nothing."""
    cin_mean, live = stats
    score = w.detach().abs().double() * cin_mean.double()[None, :, None, None]
    if live is not None:
        score = score * live[:, None, None, None]
    if whole_slice:
        score = score.sum((2, 3))
    return tuple(int(i) for i in np.unravel_index(int(torch.argmax(score)), tuple(score.shape)))


def mutations(precision_class, net, x):
    """The mutation set of a precision class for `net` on the sample positions x.  "f32": one weight element of a residual conv
    zeroed in the first and in the last block, one stem tap zeroed, the four corner points of one channel of the last block's
    output zeroed.  "f16": one whole 3x3 (cout, cin) slice of a residual conv zeroed, and the corner mutation.  Deterministic: the
    element / slice with the largest |w| x mean |input| on x, the channel with the largest corner values."""
    S = net.main_network.S
    rows, cols = [0, 0, S - 1, S - 1], [0, S - 1, 0, S - 1]
    blocks = _residual_blocks(net)
    last = len(blocks) - 1

    def corner_hook(i, y):
        if i != last:
            return y
        y = y.clone()
        c = int(torch.argmax(y[:, :, rows, cols].abs().mean((0, 2))))
        y[:, c, rows, cols] = 0.0
        return y

    def zero_at(path, idx):                       # path: (block index or None for the stem, conv attribute)
        def edit(m):
            conv = m.main_network.conv1.conv[0] if path[0] is None else getattr(_residual_blocks(m)[path[0]], path[1])
            conv.weight[idx] = 0.0
        return edit

    corner = Mutation("last block output: four corner points of one channel zeroed", hook=corner_hook)
    b0, bl, stem = blocks[0].conv_1, blocks[-1].conv_2, net.main_network.conv1.conv[0]
    if precision_class == "f32":
        i0 = _pick(b0.weight, _stats(net, x, b0, blocks[0].batchnormlize_2))
        il = _pick(bl.weight, _stats(net, x, bl))
        ist = _pick(stem.weight, _stats(net, x, stem, net.main_network.conv1))
        return [Mutation(f"first block conv_1: weight {i0} zeroed", edit=zero_at((0, "conv_1"), i0)),
                Mutation(f"last block conv_2: weight {il} zeroed", edit=zero_at((last, "conv_2"), il)),
                Mutation(f"stem: tap {ist} zeroed", edit=zero_at((None, None), ist)),
                corner]
    assert precision_class == "f16", precision_class
    isl = _pick(bl.weight, _stats(net, x, bl), whole_slice=True)
    return [Mutation(f"last block conv_2: 3x3 slice {isl} zeroed", edit=zero_at((last, "conv_2"), isl)), corner]


def reference(net, x, mode="f64", mutation=None):
    """Float64 reference of a precision mode on the positions x: "f64" (exact f32 and f32x3 paths), "half" (f16), "half_res" (f16r);
    with `mutation` applied if given.  Returns (policy, value, own) as float64 NumPy arrays."""
    m = net if mutation is None else mutation.apply(net)
    hook = None if mutation is None else mutation.hook
    if mode == "f64":
        return float64_forward(m, x, block_hook=hook)
    assert mode in ("half", "half_res"), mode
    return tuple(t.numpy() for t in half_storage_forward(m, x, half_residual=mode == "half_res", f64=True, block_hook=hook))
