"""Helper of the fp16-storage attention tests (no tests here): a torch network for any trunk program of residual and attention
blocks, assembled from oracle.net's modules under the names transgo_amd.model.pack_weights reads, and the emulation of what
net_precision 1 ("f16") computes for it.

Rounding points of the fp16-storage chain with attention (k_attention_h).  Rounded to fp16, nearest even:
  * convolutions: what oracle.net.half_storage_forward lists -- BN-folded weights and the inputs of the stem, of both convs of a
    residual block and of the value/ownership head conv (and of the policy conv where the policy head has no attention);
  * attention block: the input of the q/k/v projection -- x, or relu(bn_res_end(x)) in the policy head -- and the q|k|v weights
    (not BN-folded).
f32 inside the attention block: biases, q, k, v, energies, softmax, the output GEMM, gamma, the residual (the unrounded stream
value; in the policy head the unrounded relu(bn_res_end(x))) and the block's BN.  A residual block that follows reads
half(relu(bn1(y))) of the unrounded y; the policy conv on the attention output is f32 with f32 weights."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.net import ConvBnRelu, PreActBlock, SelfAttention, parity_weights


def arch_of(code):
    """transgo_amd.model.Arch for a code such as "RA+P", with the MainNetwork's module names (res_conv2, res_conv3, ...,
    attention_act): arch_of("RARRRARRRRAR+P") is transgo_arch()."""
    from transgo_amd.model import Arch
    kinds, _, pol = code.partition("+")
    assert pol in ("", "P")
    return Arch(kinds, [f"res_conv{i + 2}" for i in range(len(kinds))], policy_attention="attention_act" if pol else None)


class ArchBody(nn.Module):
    def __init__(self, arch, board_size, input_dim, f):
        super().__init__()
        self.S, self.arch = board_size, arch
        P = board_size * board_size
        self.conv1 = ConvBnRelu(input_dim, f)
        for kind, name in zip(arch.kinds, arch.names):
            setattr(self, name, SelfAttention(f) if kind == "A" else PreActBlock(f))
        self.bn_res_end = nn.BatchNorm2d(f)
        self.conv_val_own = ConvBnRelu(f, 2)
        self.fc_val_own = nn.Linear(2 * P, 64)
        self.fc_val = nn.Linear(64, 1)
        self.fc_own = nn.Linear(64, P)
        if arch.policy_attention:
            setattr(self, arch.policy_attention, SelfAttention(f))
        self.conv_act = ConvBnRelu(f, 4)
        self.fc_act = nn.Linear(4 * P, P + 1)

    def forward(self, x):
        P = self.S * self.S
        x = self.conv1(x)
        for name in self.arch.names:
            x = getattr(self, name)(x)
        x = F.relu(self.bn_res_end(x))
        h = F.relu(self.fc_val_own(self.conv_val_own(x).view(-1, 2 * P)))
        val = torch.tanh(self.fc_val(h))
        own = torch.tanh(self.fc_own(h))
        a = getattr(self, self.arch.policy_attention)(x) if self.arch.policy_attention else x
        act = torch.softmax(self.fc_act(self.conv_act(a).view(-1, 4 * P)), -1)
        return act, val, own


class ArchNet(nn.Module):
    """TransGoNetwork surface around ArchBody; with arch_of("RARRRARRRRAR+P") its state_dict is TransGoMain's."""

    def __init__(self, arch, board_size=9, input_dim=10, filters=128):
        super().__init__()
        self.main_network = ArchBody(arch, board_size, input_dim, filters)

    def main_prediction(self, state):
        return self.main_network(state)


def parity_arch(code, board_size=9, input_dim=10, filters=128, seed=1234, calib=None):
    """ArchNet of `code` with oracle.net.parity_weights."""
    return parity_weights(ArchNet(arch_of(code), board_size, input_dim, filters).eval(), seed, calib)


def seeded_arch(code, board_size=9, input_dim=10, filters=128, seed=1234):
    """ArchNet of `code` with torch's default init under manual_seed, BN running statistics and gains as oracle.net.seeded_tower
    draws them, attention gamma U(0.5, 1.5): the weight class of model.random_weights / random_transgo_weights, for which the
    project states its 1e-3 absolute bound of the fp16 modes."""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    net = ArchNet(arch_of(code), board_size, input_dim, filters).eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
                m.weight.copy_(1.0 + 0.1 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
            if isinstance(m, SelfAttention):
                m.gamma.copy_(0.5 + torch.rand(1, generator=g))
    return net


def arch_from_net(net):
    """The Arch of an ArchNet, or the shipped one for oracle.net.TransGoMain (same module names)."""
    body = net.main_network
    return body.arch if hasattr(body, "arch") else arch_of("RARRRARRRRAR+P")


def half_attention_forward(net, x, f64=False, block_hook=None, exact=False):
    """The fp16-storage / f32-accumulate evaluation of `net` (ArchNet or TransGoMain) with the rounding points listed at the top of
    this file, in the style of oracle.net.half_storage_forward: f64=True keeps the rounding points (and the f32 storage of folded
    parameters) but accumulates and carries everything else in float64 -- the reference of the parity tests.  block_hook(i, y) -> y
    edits the output of residual block i.  exact=True (with f64) replaces every rounding, fp16 and the f32 storage of folded
    parameters alike, by the identity: the network itself in float64.  Returns torch tensors (policy, value, own)."""
    body = net.main_network
    arch = arch_from_net(net)
    P = body.S * body.S
    dt = torch.float64 if f64 else torch.float32
    assert f64 or not exact
    q = (lambda t: t.to(dt)) if exact else (lambda t: t.half().to(dt))
    st = (lambda t: t.to(dt)) if exact else (lambda t: t.float().to(dt))       # parameters the blob stores as f32
    x = torch.as_tensor(x).to(dt)
    dense = lambda lin, t: F.linear(t, lin.weight.to(dt), lin.bias.to(dt))
    ch = lambda v: v[None, :, None, None]

    def fold(bn):
        s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        return s, bn.bias.double() - bn.running_mean.double() * s

    def conv_bn_relu(block, inp, half=True):           # ConvBnRelu with its BN folded into the (fp16, or f32) weights
        conv, bn = block.conv[0], block.conv[1]
        s, t = fold(bn)
        w = st(conv.weight.double() * s[:, None, None, None])
        b = st(conv.bias.double() * s + t)
        return F.relu(F.conv2d(inp, q(w) if half else w, b, 1, 1))

    def attention(m, xin):                             # xin: the unrounded f32 input (and residual) of the block
        n, c, w, h = xin.shape
        xh = q(xin)
        proj = lambda conv: F.conv2d(xh, q(st(conv.weight)), st(conv.bias))
        qq = proj(m.query_conv).view(n, -1, w * h).permute(0, 2, 1)
        kk = proj(m.key_conv).view(n, -1, w * h)
        att = torch.softmax(torch.bmm(qq, kk), dim=-1)
        v = proj(m.value_conv).view(n, -1, w * h)
        out = torch.bmm(v, att).view(n, c, w, h)
        s, t = fold(m.bn)
        return F.relu((st(m.gamma) * out + xin) * ch(st(s)) + ch(st(t)))

    with torch.no_grad():
        y = conv_bn_relu(body.conv1, x)
        ri = 0
        for kind, name in zip(arch.kinds, arch.names):
            b = getattr(body, name)
            if kind == "A":
                y = attention(b, y)
                continue
            s1, t1 = fold(b.batchnormlize_1)
            s2, t2 = fold(b.batchnormlize_2)
            w1 = st(b.conv_1.weight.double() * s2[:, None, None, None])
            b1 = st(b.conv_1.bias.double() * s2 + t2)
            a = q(F.relu(y * ch(st(s1)) + ch(st(t1))))
            hmid = q(F.relu(F.conv2d(a, q(w1), b1, 1, 1)))
            y = F.conv2d(hmid, q(st(b.conv_2.weight)), st(b.conv_2.bias), 1, 1) + y
            if block_hook is not None:
                y = block_hook(ri, y)
            ri += 1
        se, te = fold(body.bn_res_end)
        tail = F.relu(y * ch(st(se)) + ch(st(te)))
        z = q(tail)
        hid = F.relu(dense(body.fc_val_own, conv_bn_relu(body.conv_val_own, z).view(-1, 2 * P)))
        val = torch.tanh(dense(body.fc_val, hid))
        own = torch.tanh(dense(body.fc_own, hid))
        if arch.policy_attention:
            pc = conv_bn_relu(body.conv_act, attention(getattr(body, arch.policy_attention), tail), half=False)
        else:
            pc = conv_bn_relu(body.conv_act, z)
        act = torch.softmax(dense(body.fc_act, pc.view(-1, 4 * P)), -1)
    return act, val, own


def half_reference(net, x, mutation=None):
    """Float64 reference of "f16" on the positions x (mutation: an oracle.net.Mutation, applied first) as float64 NumPy arrays."""
    m = net if mutation is None else mutation.apply(net)
    hook = None if mutation is None else mutation.hook
    return tuple(t.numpy() for t in half_attention_forward(m, x, f64=True, block_hook=hook))


def _attentions(net):
    """(module path below main_network, module) of every attention block, trunk order, the policy head's last."""
    body, arch = net.main_network, arch_from_net(net)
    names = [n for k, n in zip(arch.kinds, arch.names) if k == "A"]
    if arch.policy_attention:
        names.append(arch.policy_attention)
    return [(n, getattr(body, n)) for n in names]


def attention_mutations(net, x, tol):
    """Attention-specific bugs as oracle.net.Mutation objects: gamma of the first trunk attention zeroed, one value_conv output
    channel zeroed, one query_conv output channel zeroed (first attention block), the policy attention's query bias zeroed (archs
    with +P).  The channel of the two channel mutations is the one with the largest effect on the float64 reference on x; a
    channel mutation whose best channel stays below 4 x tol is dropped (returned list: those that remain)."""
    from oracle.net import Mutation, parity_error
    arch = arch_from_net(net)
    atts = _attentions(net)
    first = atts[0][0]
    ref = half_reference(net, x)

    def zero(path, attr, idx=None):
        def edit(m):
            t = getattr(getattr(m.main_network, path), attr)
            t = t if isinstance(t, torch.Tensor) else t.weight
            if idx is None:
                t.zero_()
            else:
                t[idx] = 0.0
        return edit

    def zero_channel(path, conv, c):
        def edit(m):
            cv = getattr(getattr(m.main_network, path), conv)
            cv.weight[c] = 0.0
            cv.bias[c] = 0.0
        return edit

    def best_channel(path, conv, candidates):
        eff = [(parity_error(half_reference(net, x, Mutation("", edit=zero_channel(path, conv, c))), ref)[0], c) for c in candidates]
        return max(eff)

    out = []
    if "A" in arch.kinds:
        out.append(Mutation(f"{first}: gamma zeroed", edit=zero(first, "gamma")))
    # candidates: the channels with the largest weight norm (the search itself costs one reference evaluation per candidate)
    for conv, ncand in (("value_conv", 4), ("query_conv", 8)):
        w = getattr(atts[0][1], conv).weight.detach().flatten(1).norm(dim=1)
        cand = [int(c) for c in torch.argsort(w, descending=True)[:ncand]]
        eff, c = best_channel(first, conv, cand)
        if eff >= 4 * tol:
            out.append(Mutation(f"{first}.{conv}: output channel {c} zeroed", edit=zero_channel(first, conv, c)))
    if arch.policy_attention:
        def edit(m, p=arch.policy_attention):
            getattr(m.main_network, p).query_conv.bias.zero_()
        out.append(Mutation(f"{arch.policy_attention}: query bias zeroed", edit=edit))
    return out


def state_dict_np(net):
    return {k: v.detach().numpy() for k, v in net.state_dict().items()}


# ---- the weight sets both test files use (computed once per process) ---------------------------------------------------------
K = 40                       # distinct positions from play, + the empty board and the all-edges board
SHORT = ("A", "AR", "AA", "RA+P")
FULL = "RARRRARRRRAR+P"
SEED = 428                   # 300 + filters, as tests/test_gpu_net_parity.py seeds its MainNetwork
_setups = {}


def setup(code):
    """dict(net, arch, x, alt, ref, props, sens) of the parity weight set of arch `code` at 9x9, F = 128: x the K + 2 checked
    positions, alt the prefill positions, ref the float64 emulation on x, sens the emulation's own sensitivity to the order of
    summation (f32-accumulating against float64-accumulating emulation, logit space)."""
    if code not in _setups:
        from oracle.net import check_weight_properties, parity_error, parity_transgo
        from tests.test_net_reference import parity_positions
        torch.set_num_threads(8)
        x = parity_positions(9, K, 109)
        net = parity_transgo(9, 10, 128, SEED, x) if code == FULL else parity_arch(code, 9, 10, 128, SEED, x)
        ref = half_reference(net, x)
        emu32 = [t.numpy() for t in half_attention_forward(net, x)]
        _setups[code] = dict(net=net, arch=arch_of(code), x=x, alt=parity_positions(9, K + 2, 909), ref=ref,
                             props=check_weight_properties(ref), sens=parity_error(emu32, ref)[0])
    return _setups[code]


def case_mutations(code, tol):
    """The mutation set of a case: oracle.net.mutations("f16", ...) where the arch has a residual block, and the attention ones."""
    s = setup(code)
    if "muts" not in s:
        from oracle.net import mutations
        s["muts"] = (mutations("f16", s["net"], s["x"]) if "R" in code else []) + attention_mutations(s["net"], s["x"], tol)
    return s["muts"]
