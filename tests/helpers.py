"""Test-only helpers: tiny custom op tables run through the C ABI (pf_hardnet_forward_dense)."""
import ctypes
import functools
import json
import os

import torch

from panoptic_forecasting_amd import hardnet_arch as arch
from panoptic_forecasting_amd import lib as _lib
from panoptic_forecasting_amd import packing


class MiniSpec:
    """An op table built by hand (same fields packing.pack_blob reads from hardnet_arch.Spec)."""

    def __init__(self, in_ch):
        self.in_ch, self.n_cls = in_ch, 1
        self.tensors = [arch.Tensor('input', in_ch)]
        self.ops = []
        self.input_tensor = 0

    def tensor(self, name, ch):
        self.tensors.append(arch.Tensor(name, ch))
        return len(self.tensors) - 1

    def conv(self, name, srcs, cout, k, stride=1, dst=None, dst_choff=0, relu=True, bn=False):
        cin = sum(s.ch for s in srcs)
        if dst is None:
            dst = self.tensor(name, cout)
        self.ops.append(arch.Op(arch.OP_CONV, name, srcs, dst, dst_choff, cin, cout, k, stride, relu, bn=bn))
        return dst

    def stem(self, name, T, n_cls):
        """the fused one-hot stem (pf_bg_forward): 3x3 stride 2 + ReLU over the T*(n_cls+1) input channels the kernels never build,
        into a 16-channel tensor of its own"""
        cin = T * (n_cls + 1)
        assert cin == self.in_ch and not self.ops
        self.n_cls = n_cls
        dst = self.tensor(name, 16)
        self.ops.append(arch.Op(arch.OP_STEM, name, [arch.Src(0, 0, cin)], dst, 0, cin, 16, 3, 2, True, bn=False))
        return dst

    def head(self, logits_t):
        ch = self.tensors[logits_t].channels
        self.n_cls = ch
        self.ops.append(arch.Op(arch.OP_HEAD, 'head', [arch.Src(logits_t, 0, ch)], logits_t, 0, ch, ch, 1, 1, False, False))

    def pool(self, name, src_t):
        ch = self.tensors[src_t].channels
        d = self.tensor(name, ch)
        self.ops.append(arch.Op(arch.OP_POOL, name, [arch.Src(src_t, 0, ch)], d, 0, ch, ch, 2, 2, False, False))
        return d

    def upsample(self, name, src_t, like_t):
        ch = self.tensors[src_t].channels
        d = self.tensor(name, ch)
        self.ops.append(arch.Op(arch.OP_UPSAMPLE, name, [arch.Src(src_t, 0, ch),
                                                         arch.Src(like_t, 0, self.tensors[like_t].channels)],
                                d, 0, ch, ch, 1, 1, False, False))
        return d

    def conv_ops(self):
        return [o for o in self.ops if o.kind in (arch.OP_STEM, arch.OP_CONV)]


class MiniNet:
    def __init__(self, spec, params):
        L = _lib.load()
        blob = packing.pack_blob(None, spec.in_ch, spec.n_cls, spec=spec, params=params)
        self._buf = ctypes.create_string_buffer(blob, len(blob))
        self.plan = ctypes.c_void_p()
        _lib.check(L.pf_hardnet_plan_create(self._buf, len(blob), spec.in_ch, spec.n_cls, ctypes.byref(self.plan)),
                   'pf_hardnet_plan_create')
        self.spec = spec

    def _workspace(self, x):
        """a zeroed workspace for an input of x's shape (kept as self.ws) -> (the library, contiguous x, b, h, w)"""
        L = _lib.load()
        b, _, h, w = x.shape
        need = ctypes.c_size_t()
        _lib.check(L.pf_hardnet_workspace(self.plan, b, h, w, ctypes.byref(need)), 'pf_hardnet_workspace')
        self.ws = torch.zeros(need.value, dtype=torch.uint8, device=x.device)
        self.bhw = (b, h, w)
        return L, x.contiguous(), b, h, w

    def run(self, x):
        L, x, b, h, w = self._workspace(x)
        rc = L.pf_hardnet_forward_dense(self.plan, x.data_ptr(), b, h, w, 0, 0, None, 0, None, None,
                                        self.ws.data_ptr(), self.ws.numel(), _lib.stream_ptr())
        _lib.check(rc, 'pf_hardnet_forward_dense')
        torch.cuda.synchronize()
        return self

    def run_head(self, x, out_h, out_w, seg_dtype=torch.uint8, want_logits=True):
        """the forward with the head's outputs requested: (rc, seg [B, out_h, out_w] of ``seg_dtype`` (uint8 / int64), out_logits
        [B, C, out_h, out_w] or None, out_orig_logits = the head's input as the library copies it out).  The outputs are
        pre-filled with values no kernel writes (label 250, NaN), so a pixel left out shows"""
        L, x, b, h, w = self._workspace(x)
        c = self.spec.n_cls
        assert seg_dtype in (torch.uint8, torch.int64)
        seg = torch.full((b, out_h, out_w), 250, dtype=seg_dtype, device=x.device)
        logits = torch.full((b, c, out_h, out_w), float('nan'), device=x.device) if want_logits else None
        orig = torch.full((b, c, h, w), float('nan'), device=x.device)
        rc = L.pf_hardnet_forward_dense(self.plan, x.data_ptr(), b, h, w, out_h, out_w, seg.data_ptr(), int(seg_dtype == torch.int64),
                                        logits.data_ptr() if want_logits else None, orig.data_ptr(), self.ws.data_ptr(),
                                        self.ws.numel(), _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, seg, logits, orig

    def run_bg(self, seg, depth, mask, mean, std, hop_flags, min_depth, max_depth, out_h, out_w):
        """pf_bg_forward on seg [B, T, H, W] (uint8 / int64), depth (fp32) and mask (uint8; None under PF_HOP_DEPTH_U16) -> rc.  The
        outputs are pre-filled as in run_head and kept as self.out = (seg, out_logits, out_orig_logits)"""
        L, seg, b, h, w = self._workspace(seg)
        t, c = seg.shape[1], self.spec.n_cls
        assert seg.dtype in (torch.uint8, torch.int64) and depth.dtype == torch.float32 and (mask is None or mask.dtype == torch.uint8)
        depth = depth.contiguous()
        mask = None if mask is None else mask.contiguous()
        oh, ow = (h + 1) // 2, (w + 1) // 2
        for op in self.spec.ops[1:]:
            if op.kind == arch.OP_CONV and op.stride == 2:
                oh, ow = (oh + 1) // 2, (ow + 1) // 2
        out_seg = torch.full((b, out_h, out_w), 250, dtype=torch.uint8, device=seg.device)
        logits = torch.full((b, c, out_h, out_w), float('nan'), device=seg.device)
        orig = torch.full((b, c, oh, ow), float('nan'), device=seg.device)
        rc = L.pf_bg_forward(self.plan, seg.data_ptr(), int(seg.dtype == torch.int64), depth.data_ptr(),
                             None if mask is None else mask.data_ptr(), float(mean), float(std), int(hop_flags), float(min_depth),
                             float(max_depth), b, t, h, w, out_h, out_w, out_seg.data_ptr(), 0, logits.data_ptr(), orig.data_ptr(),
                             self.ws.data_ptr(), self.ws.numel(), _lib.stream_ptr())
        torch.cuda.synchronize()
        self.out = (out_seg, logits, orig)
        return rc

    def tensor(self, name):
        return view_tensor(self.plan, self.ws, name, *self.bhw)

    def stored_tensor(self, name):
        """the tensor as the last forward stored it, if that was fp32 NCHW: in the plan's own units (times its per-channel powers
        of two), where tensor() hands out the caller's"""
        L = _lib.load()
        b, h, w = self.bhw
        off, c, th, tw = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.check(L.pf_hardnet_tensor_view(self.plan, name.encode(), b, h, w, ctypes.byref(off), ctypes.byref(c), ctypes.byref(th),
                                            ctypes.byref(tw)), 'pf_hardnet_tensor_view')
        n = b * c.value * th.value * tw.value
        stored = self.ws[off.value:off.value + 4 * n].view(torch.float32).view(b, c.value, th.value, tw.value).clone()
        # the guard: what pf_hardnet_tensor_read hands out is this times one power of two per channel - true of fp32 NCHW storage,
        # not of the packed-pair bytes of the same region read as floats
        x = self.tensor(name)
        assert torch.equal(x == 0, stored == 0), 'tensor %s is not stored as fp32 NCHW' % name
        for ch in range(c.value):
            nz = stored[:, ch] != 0
            r = (x[:, ch][nz] / stored[:, ch][nz]).unique()
            assert len(r) <= 1 and bool((torch.frexp(r)[0] == 0.5).all()), 'tensor %s is not stored as fp32 NCHW' % name
        return stored

    def set_option(self, name, value):
        _lib.check(_lib.load().pf_hardnet_plan_set_option(self.plan, name.encode(), int(value)), 'pf_hardnet_plan_set_option')
        return self

    def status(self):
        """status word of the last forward (include/pfhip.h: PF_STATUS_RANGE = 1), through the C entry point"""
        st = ctypes.c_uint(0xFFFFFFFF)
        _lib.check(_lib.load().pf_hardnet_status(self.ws.data_ptr(), ctypes.byref(st), _lib.stream_ptr()), 'pf_hardnet_status')
        assert st.value == int(self.ws[:4].view(torch.int32).item())
        return st.value

    def close(self):
        _lib.load().pf_hardnet_plan_destroy(self.plan)


def view_tensor(plan, ws, name, b, h, w):
    L = _lib.load()
    off, c, th, tw = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(L.pf_hardnet_tensor_view(plan, name.encode(), b, h, w, ctypes.byref(off), ctypes.byref(c),
                                        ctypes.byref(th), ctypes.byref(tw)), 'pf_hardnet_tensor_view')
    out = torch.empty(b, c.value, th.value, tw.value, dtype=torch.float32, device=ws.device)
    # fp32 copy of the tensor whatever layout the last forward kept it in (packed-pair tensors: hi + mid)
    _lib.check(L.pf_hardnet_tensor_read(plan, name.encode(), b, h, w, ws.data_ptr(), out.data_ptr(), _lib.stream_ptr()),
               'pf_hardnet_tensor_read')
    torch.cuda.synchronize()
    return out


SLICES = [('A', 0, 10), ('B', 10, 10), ('C', 20, 18)]


def slices_net(g, k, stride, src='t0'):
    """t0 = conv3x3(input) (src = 't0' only); A, B, C = three k x k convs (stride `stride`) over t0 - or, src = 'input', over the fp32 network input - into
    the slices 0 / 10 / 20 of `out` (38 channels: block growth (10, 18)); fin = a 3x3 conv over out, the packed-pair reader that makes
    the plan keep `out` in that layout.  Returns the spec and its parameters"""
    S = arch.Src
    spec = MiniSpec(12)
    from_t, cin, shapes = 0, 12, []
    if src == 't0':
        from_t, cin, shapes = spec.conv('t0', [S(0, 0, 12)], 24, 3), 24, [('t0', 12, 24, 3)]
    out = spec.tensor('out', 38)
    for name, off, ch in SLICES:
        spec.conv(name, [S(from_t, 0, cin)], ch, k, stride=stride, dst=out, dst_choff=off)
        shapes.append((name, cin, ch, k))
    spec.conv('fin', [S(out, 0, 38)], 9, 3, relu=False)
    shapes.append(('fin', 38, 9, 3))
    P = {n: (torch.randn(co, ci, kk, kk, generator=g) / (ci * kk * kk) ** 0.5, torch.randn(co, generator=g) * 0.5) for n, ci, co, kk in shapes}
    return spec, P


def pooled_net(g, cout=18):
    """dn = a 1x1 conv with ReLU over the fp32 network input, pl = its 2x2 average pool, fin = a 3x3 conv over pl: the packed-pair reader
    that makes an fp32-source kernel store the pooled tensor (cout = 18: half of its last group) as packed pairs"""
    S = arch.Src
    spec = MiniSpec(12)
    pl = spec.pool('pl', spec.conv('dn', [S(0, 0, 12)], cout, 1))
    spec.conv('fin', [S(pl, 0, cout)], 9, 3, relu=False)
    shapes = [('dn', 12, cout, 1), ('fin', cout, 9, 3)]
    P = {n: (torch.randn(co, ci, kk, kk, generator=g) / (ci * kk * kk) ** 0.5, torch.randn(co, generator=g) * 0.5) for n, ci, co, kk in shapes}
    return spec, P


class MiniTrain:
    """A hand-built op table through the training entry points (pf_train_*), dense input.  ``params``: {op name: dict(w=,
    gamma=, beta=, mean=, var=) for conv+BN ops, dict(w=, b=) for plain convs} (CPU tensors)."""

    def __init__(self, spec, params):
        L = _lib.load()
        dummy = {op.name: (torch.zeros(op.cout, op.cin, op.k, op.k), torch.zeros(op.cout)) for op in spec.conv_ops()}
        blob = packing.pack_blob(None, spec.in_ch, spec.n_cls, spec=spec, params=dummy)
        self._buf = ctypes.create_string_buffer(blob, len(blob))
        self.t = ctypes.c_void_p()
        _lib.check(L.pf_train_create(self._buf, len(blob), spec.in_ch, spec.n_cls, ctypes.byref(self.t)), 'pf_train_create')
        n = ctypes.c_size_t()
        _lib.check(L.pf_train_param_count(self.t, ctypes.byref(n)), 'pf_train_param_count')
        self.spec = spec
        host = torch.zeros(n.value)
        self.slots = {}
        for i, op in enumerate(spec.ops):
            if op.kind not in (arch.OP_STEM, arch.OP_CONV):
                continue
            wo, ao, bn = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int()
            _lib.check(L.pf_train_param_layout(self.t, i, ctypes.byref(wo), ctypes.byref(ao), ctypes.byref(bn)), 'pf_train_param_layout')
            assert bool(bn.value) == bool(op.bn)
            pr = params[op.name]
            nw = op.cout * op.cin * op.k * op.k
            host[wo.value:wo.value + nw] = pr['w'].reshape(-1)
            self.slots[op.name + '.w'] = (wo.value, (op.cout, op.cin, op.k, op.k))
            names = ('gamma', 'beta', 'mean', 'var') if op.bn else ('b',)
            for j, nm in enumerate(names):
                host[ao.value + j * op.cout:ao.value + (j + 1) * op.cout] = pr[nm]
                self.slots[op.name + '.' + nm] = (ao.value + j * op.cout, (op.cout,))
        self.theta = host.cuda()
        self.grad = torch.zeros_like(self.theta)

    def step(self, x, labels, loss_scale=1.0):
        L = _lib.load()
        b, _, h, w = x.shape
        oh, ow = labels.shape[-2:]
        need = ctypes.c_size_t()
        _lib.check(L.pf_train_workspace(self.t, b, h, w, oh, ow, ctypes.byref(need)), 'pf_train_workspace')
        self.ws = torch.zeros(need.value, dtype=torch.uint8, device='cuda')
        self.out3 = torch.zeros(3, dtype=torch.float64, device='cuda')
        x, labels = x.contiguous(), labels.contiguous()
        rc = L.pf_train_forward_backward(self.t, self.theta.data_ptr(), self.grad.data_ptr(), 0, None, 0, None, None, 0.0, 1.0, 1,
                                         x.data_ptr(), b, h, w, labels.data_ptr(), int(labels.dtype == torch.int64), oh, ow, 255,
                                         float(loss_scale), 0.1, 1e-5, 1, self.out3.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                         _lib.stream_ptr())
        _lib.check(rc, 'pf_train_forward_backward')
        torch.cuda.synchronize()
        self.dims = (b, h, w, oh, ow)
        return float(self.out3[0] / self.out3[1])

    def param(self, name, grad=False):
        off, shape = self.slots[name]
        n = 1
        for d in shape:
            n *= d
        return (self.grad if grad else self.theta)[off:off + n].view(shape)

    def tensor(self, name, grad=False):
        L = _lib.load()
        off, c, th, tw = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        b = self.dims[0]
        _lib.check(L.pf_train_tensor_view(self.t, name.encode(), int(grad), *self.dims, ctypes.byref(off), ctypes.byref(c),
                                          ctypes.byref(th), ctypes.byref(tw)), 'pf_train_tensor_view')
        n = b * c.value * th.value * tw.value
        return self.ws[off.value:off.value + 4 * n].view(torch.float32).view(b, c.value, th.value, tw.value)

    def path_stats(self):
        """pf_train_path_stats of the last step (include/pfhip.h: [0] table, [1] cost model, [2] measured, ..., [7] packed pairs)"""
        buf, n = (ctypes.c_int * 8)(), ctypes.c_int()
        _lib.check(_lib.load().pf_train_path_stats(self.t, buf, 8, ctypes.byref(n)), 'pf_train_path_stats')
        return list(buf)

    def close(self):
        _lib.load().pf_train_destroy(self.t)


def mini_net():
    """Every op kind of the training path in one small, well-conditioned network: stride-2 stem, 3x3 convs with one and
    two input ranges, a conv writing into a slice of a wider tensor, 1x1 conv, pool, upsample + 1x1 over [up, skip],
    plain final conv, bilinear head."""
    sp = MiniSpec(6)
    S = arch.Src
    c0 = sp.conv('c0', [S(0, 0, 6)], 16, 3, stride=2, bn=True)
    c1 = sp.conv('c1', [S(c0, 0, 16)], 24, 3, bn=True)
    cat = sp.tensor('cat', 28 + 10 + 12)
    sp.conv('c2', [S(c1, 0, 24), S(c0, 0, 16)], 28, 3, dst=cat, dst_choff=10, bn=True)
    sp.conv('c2b', [S(c1, 4, 18)], 10, 3, dst=cat, dst_choff=0, bn=True)
    # like the last layer of a HarDBlock: three ranges, the first one a slice of the tensor it writes into
    sp.conv('c2c', [S(cat, 0, 10), S(c1, 0, 24), S(c0, 0, 16)], 12, 3, dst=cat, dst_choff=38, bn=True)
    c3 = sp.conv('c3', [S(cat, 0, 50)], 20, 1, bn=True)
    p = sp.pool('p', c3)
    c4 = sp.conv('c4', [S(p, 0, 20)], 34, 3, bn=True)
    up = sp.upsample('up', c4, c3)
    c5 = sp.conv('c5', [S(up, 0, 34), S(c3, 0, 20)], 22, 1, bn=True)
    fin = sp.conv('fin', [S(c5, 0, 22), S(cat, 10, 28)], 11, 1, relu=False, bn=False)
    sp.head(fin)
    return sp


def train_plan_tables(blob, in_ch, n_cls, b, h, w, out_h, out_w):
    """pf_debug_train_plan (no GPU) under the process-wide options as they are: (regions [n][4] = kind, index, offset, bytes;
    steps [m][5]; (dy slots, side streams)) - include/pfhip.h documents the rows"""
    import numpy as np
    L = _lib.load()
    buf = ctypes.create_string_buffer(blob, len(blob))
    nr, ns, consts = ctypes.c_int(), ctypes.c_int(), (ctypes.c_int * 2)()
    args = (buf, len(blob), in_ch, n_cls, b, h, w, out_h, out_w)
    _lib.check(L.pf_debug_train_plan(*args, None, 0, ctypes.byref(nr), None, 0, ctypes.byref(ns), consts), 'pf_debug_train_plan')
    regions, steps = np.zeros((nr.value, 4), dtype=np.int64), np.zeros((ns.value, 5), dtype=np.int32)
    _lib.check(L.pf_debug_train_plan(*args, regions.ctypes.data, nr.value, ctypes.byref(nr), steps.ctypes.data, ns.value, ctypes.byref(ns),
                                     consts), 'pf_debug_train_plan')
    assert (nr.value, ns.value) == (len(regions), len(steps))
    return regions, steps, tuple(consts)


def plan_path_stats(steps):
    """pf_train_path_stats as a step counts it: per slot, the steps of the table whose stats bits have that bit"""
    bits = steps[steps[:, 0] == 0][:, 4]
    return [int(((bits >> k) & 1).sum()) for k in range(8)]


def mini_torch(sp, params, x, labels, dtype=torch.float64, pre=None):
    """The same op table through torch autograd on the CPU, with gradients of every tensor retained: in float64 the checker, in
    float32 (ATen) the yardstick of what fp32 rounding alone does.  ``pre``: a dict that receives every conv's output before
    BatchNorm / ReLU (retained: ``.grad`` is the gradient the weight gradient is formed from).  The running statistics come back
    with the leaves: ``leaves[op]['mean']`` / ``['var']`` are copies of the caller's buffers in ``dtype`` that the BatchNorm of
    the step has updated (momentum 0.1, unbiased variance); ``params`` itself is not touched."""
    import torch.nn.functional as F
    leaves = {n: {k: v.to(dtype).clone().requires_grad_(k in ('w', 'gamma', 'beta', 'b')) for k, v in pr.items()} for n, pr in params.items()}
    parts = {}           # tensor index -> {choff: produced slice}
    whole = {0: x.to(dtype)}
    kept = {}

    def get(src):
        if src.tensor in whole:
            return whole[src.tensor][:, src.choff:src.choff + src.ch]
        pr = parts[src.tensor]
        if src.choff in pr and pr[src.choff].shape[1] == src.ch and sum(p.shape[1] for p in pr.values()) < sp.tensors[src.tensor].channels:
            return pr[src.choff]                       # a slice read while the tensor is still being filled
        t = torch.cat([pr[k] for k in sorted(pr)], 1)
        assert t.shape[1] == sp.tensors[src.tensor].channels
        whole[src.tensor] = t
        return t[:, src.choff:src.choff + src.ch]

    logits = None
    for op in sp.ops:
        if op.kind in (arch.OP_STEM, arch.OP_CONV):
            xin = torch.cat([get(s) for s in op.srcs], 1)
            pr = leaves[op.name]
            y = F.conv2d(xin, pr['w'], None if op.bn else pr['b'], stride=op.stride, padding=op.k // 2)
            if pre is not None:
                y.retain_grad()
                pre[op.name] = y
            if op.bn:
                y = F.batch_norm(y, pr['mean'], pr['var'], pr['gamma'], pr['beta'], training=True, momentum=0.1, eps=1e-5)
            if op.relu:
                y = F.relu(y)
            if op.cout == sp.tensors[op.dst].channels:
                y.retain_grad()
                whole[op.dst] = y
                kept[sp.tensors[op.dst].name] = y
            else:
                y.retain_grad()
                parts.setdefault(op.dst, {})[op.dst_choff] = y
                kept['%s@%d' % (sp.tensors[op.dst].name, op.dst_choff)] = y
        elif op.kind == arch.OP_POOL:
            whole[op.dst] = F.avg_pool2d(get(op.srcs[0]), 2, 2)
            whole[op.dst].retain_grad()
            kept[sp.tensors[op.dst].name] = whole[op.dst]
        elif op.kind == arch.OP_UPSAMPLE:
            like = get(op.srcs[1])
            whole[op.dst] = F.interpolate(get(op.srcs[0]), size=like.shape[-2:], mode='bilinear', align_corners=True)
            whole[op.dst].retain_grad()
            kept[sp.tensors[op.dst].name] = whole[op.dst]
        else:
            logits = get(op.srcs[0])
    full = F.interpolate(logits, size=labels.shape[-2:], mode='bilinear', align_corners=True)
    loss = F.cross_entropy(full, labels.long(), ignore_index=255)
    loss.backward()
    return float(loss.detach()), leaves, kept


# ---- the single-layer probe: dense input (6 channels) -> a (-> a2) -> L -> fin -> head, one layer L under test at a time.
#      a / a2: 3x3 stride 1, BatchNorm + ReLU, so that L reads tensors some op produced and their gradients are computed.  L has NO
#      ReLU: neither dW_L, dgamma_L / dbeta_L nor the gradient arriving at a's output then depends on a ReLU mask that could flip
#      between fp32 and float64, so every compared quantity is well conditioned (unlike a deeper net's).  fin: 1x1 to n_cls with bias.
class Probe:
    """One probe case.  ``srcs``: L's input ranges, [('a' | 'a2', first channel, channels), ...]; ``ca`` / ``ca2``: channels of a / a2
    (ca2 = 0: no a2); ``slot``: L writes channels [10, 10 + cout) of a wider tensor whose first 10 channels a 1x1 conv + BatchNorm
    ``side`` over a produces (a's gradient then has a storing and an accumulating writer); ``fin_a`` = (first channel, channels): fin reads that slice of a beside L's
    output (stride 1), so those channels of a's gradient are written before L's backward pass gets to them; ``size``: L's input size;
    ``dead``: the labels of image 0 are all ignored.

    ``cond``: prescribed statistics of L's conv output y, on top of the data every case gets (which is drawn first and unchanged
    where ``cond`` is None).  L must be a 1x1 stride-1 conv + BatchNorm: a 3x3 layer's zero-padded border sees 6/9 of the mean,
    which brings |mean| / std back to about 4.
      'ill': every channel of y at |mean| / std of about ILL_RATIO.  beta of a (a2) is the constant ILL_RATIO / sqrt(cin) > 0, so
             their ReLU cuts next to nothing and every input channel of L has that mean and a std of gamma; L's weights are
             (1 + 0.1 randn) / sqrt(cin), so a channel of y has mean ~ beta * sqrt(cin) and std ~ sqrt(E gamma^2) ~ 1.04.
      'degenerate': rows 0, 1 of L's weight are zero (y = 0, var = 0, invstd = 1 / sqrt(eps)), rows 2, 3 are scaled by 1e-6
             (var << eps); the other rows stay as drawn.
    ``rstats``: L's running statistics after the step are compared too ('rmean L', 'rvar L').  They start at 0 (the variance
    too), so each is 0.1 x the batch statistic and its relative error is the statistic's."""

    ILL_RATIO = 300.0

    def __init__(self, name, k, stride, srcs, cout, size, ca, ca2=0, bn=True, slot=False, b=2, n_cls=11, u8=False, dead=False, fin_a=None,
                 cond=None, rstats=False):
        self.name, self.k, self.stride, self.cout, self.size, self.ca, self.ca2 = name, k, stride, cout, tuple(size), ca, ca2
        self.srcs = [(t, c0, n) for t, c0, n in srcs]
        self.bn, self.slot, self.b, self.n_cls, self.u8, self.dead, self.fin_a = bn, slot, b, n_cls, u8, dead, fin_a
        self.cond, self.rstats = cond, rstats
        assert cond in (None, 'ill', 'degenerate')
        assert (cond is None and not rstats) or (k == 1 and stride == 1 and bn)
        assert cond != 'degenerate' or cout >= 6
        assert (not slot and not fin_a) or stride == 1
        for t, c0, n in self.srcs:
            assert c0 + n <= (ca if t == 'a' else ca2), (name, t, c0, n)

    @property
    def cin(self):
        return sum(n for _, _, n in self.srcs)

    def spec(self):
        sp = MiniSpec(6)
        S = arch.Src
        t = {'a': sp.conv('a', [S(0, 0, 6)], self.ca, 3, bn=True)}
        if self.ca2:
            t['a2'] = sp.conv('a2', [S(0, 0, 6)], self.ca2, 3, bn=True)
        srcs = [S(t[n], c0, ch) for n, c0, ch in self.srcs]
        more = [S(t['a'], *self.fin_a)] if self.fin_a else []
        if self.slot:
            wide = sp.tensor('wide', 10 + self.cout)
            sp.conv('side', [S(t['a'], 0, self.ca)], 10, 1, dst=wide, dst_choff=0, relu=False, bn=True)
            sp.conv('L', srcs, self.cout, self.k, stride=self.stride, dst=wide, dst_choff=10, relu=False, bn=self.bn)
            fin = sp.conv('fin', [S(wide, 0, 10 + self.cout)] + more, self.n_cls, 1, relu=False, bn=False)
        else:
            lt = sp.conv('L', srcs, self.cout, self.k, stride=self.stride, relu=False, bn=self.bn)
            fin = sp.conv('fin', [S(lt, 0, self.cout)] + more, self.n_cls, 1, relu=False, bn=False)
        sp.head(fin)
        return sp

    def data(self):
        """(params, x, labels): CPU tensors, a function of the case alone"""
        sp = self.spec()
        g = torch.Generator().manual_seed(1000 + sum(ord(c) * (i + 1) for i, c in enumerate(self.name)) % 9973)
        params = {}
        for op in sp.conv_ops():
            pr = {'w': torch.randn(op.cout, op.cin, op.k, op.k, generator=g) * (2.0 / (op.cin * op.k * op.k)) ** 0.5}
            if op.bn:
                pr.update(gamma=torch.rand(op.cout, generator=g) + 0.5, beta=torch.randn(op.cout, generator=g) * 0.2,
                          mean=torch.zeros(op.cout), var=torch.ones(op.cout))
            else:
                pr['b'] = torch.randn(op.cout, generator=g) * 0.1
            params[op.name] = pr
        h, w = self.size
        x = torch.randn(self.b, 6, h, w, generator=g)
        oh, ow = (h + self.stride - 1) // self.stride, (w + self.stride - 1) // self.stride
        lab = torch.randint(0, self.n_cls + 1, (self.b, 2 * oh - 3, 2 * ow + 1), generator=g)
        lab[lab == self.n_cls] = 255
        if self.dead:
            lab[0] = 255
        # prescribed statistics: drawn after (and besides) everything above, so a case without them gets the data it always got
        if self.cond == 'ill':
            for nm in ('a', 'a2')[:1 + bool(self.ca2)]:
                params[nm]['beta'] = torch.full((params[nm]['beta'].numel(),), self.ILL_RATIO / self.cin ** 0.5)
            params['L']['w'] = (1.0 + 0.1 * torch.randn(self.cout, self.cin, 1, 1, generator=g)) / self.cin ** 0.5
        elif self.cond == 'degenerate':
            params['L']['w'][0:2] = 0.0
            params['L']['w'][2:4] *= 1e-6
        if self.rstats:
            params['L']['var'] = torch.zeros(self.cout)
        return params, x, (lab.to(torch.uint8) if self.u8 else lab)

    def quantities(self, loss, leaves, kept):
        """what a case compares, out of mini_torch's result: {name: float64 CPU tensor}"""
        q = {'loss': torch.tensor([loss], dtype=torch.float64), 'act a': kept['a'].detach(), 'grad a': kept['a'].grad}
        if self.ca2:
            q['act a2'], q['grad a2'] = kept['a2'].detach(), kept['a2'].grad
        q['act L'] = kept['wide@10' if self.slot else 'L'].detach()
        for nm in ('w', 'gamma', 'beta') if self.bn else ('w', 'b'):
            q['d%s L' % nm] = leaves['L'][nm].grad
        if self.rstats:
            q['rmean L'], q['rvar L'] = leaves['L']['mean'].detach(), leaves['L']['var'].detach()
        return {k: v.double() for k, v in q.items()}

    def quantities_hip(self, net, loss):
        q = {'loss': torch.tensor([loss], dtype=torch.float64), 'act a': net.tensor('a'), 'grad a': net.tensor('a', grad=True)}
        if self.ca2:
            q['act a2'], q['grad a2'] = net.tensor('a2'), net.tensor('a2', grad=True)
        q['act L'] = net.tensor('wide')[:, 10:10 + self.cout] if self.slot else net.tensor('L')
        for nm in ('w', 'gamma', 'beta') if self.bn else ('w', 'b'):
            q['d%s L' % nm] = net.param('L.' + nm, grad=True)
        if self.rstats:
            q['rmean L'], q['rvar L'] = net.param('L.mean'), net.param('L.var')      # theta after the step
        return {k: v.detach().cpu().double() for k, v in q.items()}


@functools.lru_cache(maxsize=None)
def _probe_reference(case):
    params, x, lab = case.data()
    sp = case.spec()
    pre = {}
    out = tuple(case.quantities(*mini_torch(sp, params, x, lab, dtype=dt, pre=pre if dt is torch.float64 else None))
                for dt in (torch.float64, torch.float32))
    y = pre['L'].detach().transpose(0, 1).reshape(case.cout, -1)
    return out + (y.mean(1).abs() / y.std(1, unbiased=False).clamp_min(1e-300),)


def probe_reference(case):
    """(float64 autograd, fp32 ATen autograd) quantities of a case - computed once per case and process, never modified"""
    return _probe_reference(case)[:2]


def probe_mean_over_std(case):
    """|mean| / std per channel of L's conv output before BatchNorm, of the float64 reference: what an ill-conditioned case is
    about (and asserts, so that it stays one)"""
    return _probe_reference(case)[2]


# the two criteria of the probe.  PROBE_REL: the project's kernel-level bar (relative L2; activations and the loss 1e-5).  The
# elementwise one: e(X) = max|X - X64| / max|X64| of the subject at most max(M * e of fp32 ATen, floor).  PROBE_M_CAP /
# PROBE_FLOOR_CAP are the largest values a test may use: with them the bar on dW stays <= 4.5e-5, a fifth of the smallest error one
# lost pixel of a weight gradient makes (tests/test_train_host.py: the bar bites)
PROBE_M_CAP, PROBE_FLOOR_CAP = 32.0, 2e-5


def probe_rel_bar(name):
    return 1e-5 if name.startswith('act') or name == 'loss' else 1e-4


def probe_distances(got, ref64, ref32):
    """per quantity: e of the subject, e of fp32 ATen, relative L2 of the subject"""
    out = {}
    for k, r in ref64.items():
        mx = float(r.abs().max()) + 1e-300
        out[k] = {'e_hip': float((got[k] - r).abs().max()) / mx, 'e_aten': float((ref32[k] - r).abs().max()) / mx,
                  'rel_hip': float((got[k] - r).norm() / (r.norm() + 1e-300))}
    return out


def probe_failures(dist, m, floor, rel_l2=True):
    """[(quantity, which criterion, value, bar)] of a case's distances.  ``rel_l2=False`` leaves the fixed relative-L2 bars out:
    for the cases with ill-conditioned channel statistics (Probe: cond='ill'), where fp32 ATen itself is at 1.7e-5 on the
    activation (|mean| / std = 300 costs every fp32 value of y 300 x 2^-24 of the std before any kernel touches it), so a bar of
    1e-5 would test the data, not the kernel.  The elementwise criterion scales with what fp32 ATen does and stays"""
    assert 1.0 <= m <= PROBE_M_CAP and 0.0 <= floor <= PROBE_FLOOR_CAP
    bad = []
    for k, d in dist.items():
        if rel_l2 and not d['rel_hip'] <= probe_rel_bar(k):
            bad.append((k, 'rel. L2', d['rel_hip'], probe_rel_bar(k)))
        bar = max(m * d['e_aten'], floor)
        if not d['e_hip'] <= bar:
            bad.append((k, 'elementwise', d['e_hip'], bar))
    return bad


def probe_record(case_id, dist, kernels):
    """train_layer_probe_dist.json in the scratch directory the suite's other measured reports go to (tests/test_gpu_precision.py:
    REPORT): e_hip / e_aten (and the relative L2) per case and quantity, and the kernels the case ran.  The run on MI355X is kept
    as profiles/train_layer_probe_dist.json: M and floor of tests/test_gpu_train_layers.py come from it"""
    _merge_report('train_layer_probe_dist.json', case_id,
                  {'e': {k: {n: float('%.4g' % v) for n, v in d.items()} for k, d in dist.items()}, 'kernels': list(kernels)})


def _merge_report(name, key, entry):
    """set ``key`` of the JSON object in file ``name`` of the suite's scratch report directory (tests/test_gpu_precision.py: REPORT)"""
    from test_gpu_precision import REPORT
    path = os.path.join(os.path.dirname(REPORT), name)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data[key] = entry
    with open(path, 'w') as f:
        json.dump(data, f, indent=0, sort_keys=True)


def head_probe_record(case_id, entry):
    """head_probe_dist.json next to the other measured reports (probe_record above): per case of tests/test_gpu_head.py the worst
    err / (u*M), the near-tie count and the kernel that ran.  The run on MI355X is kept as profiles/head_probe_dist.json"""
    _merge_report('head_probe_dist.json', case_id, entry)


def stem_probe_record(case_id, entry):
    """stem_probe_dist.json next to the other measured reports: per case of tests/test_gpu_stem.py the worst err / bar of every
    run (hop flags, parameter set) and the kernels that ran"""
    _merge_report('stem_probe_dist.json', case_id, entry)


def fg_probe_record(case_id, entry):
    """fg_probe_dist.json next to the other measured reports: per case of tests/test_gpu_fg_stages.py the worst err / bar and
    the terms the bar was made of.  The run on MI355X is kept as profiles/fg_probe_dist.json"""
    _merge_report('fg_probe_dist.json', case_id, entry)
