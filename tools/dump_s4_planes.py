"""Digest of what the packed-pair writers store (GPU): `python tools/dump_s4_planes.py [LIBPFHIP.so ...]` runs a fixed list of MiniNet
cases (tests/helpers.py; the nets of the fold, share, pair and store tests) and one training step and prints, per case, the profile labels' kernels and per tensor
of the op table the SHA-256 of its raw bytes in the workspace (both terms of every channel group where it is stored as packed pairs: the
slot_planes reader of tests/test_gpu_fold_final.py over all groups) and of its fp32 read-out (pf_hardnet_tensor_read).  A tensor the plan
elided prints `elided`.  With one library (or none: the built one) the lines go to stdout; with several each library runs in a fresh child
process through PF_LIBPFHIP and the outputs are compared: `same` / `DIFFERENT` per library against the first, exit status 1 on a difference.
Two builds store the same bits exactly when their outputs are equal: profiles/s4_store_unify.md."""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def cases():
    """[(name, (spec, params), input [b, c, h, w] seed-fixed, plan options, force_conv arguments, process-wide options)]"""
    import torch
    from test_fold_down_host import down_net
    from test_fold_final_host import tail_net
    from test_fold_wide_host import lo_net
    from helpers import pooled_net, slices_net
    from test_gpu_conv import _block_net
    from test_gpu_share_s import pair_net

    def x(seed, b, h, w):
        g = torch.Generator().manual_seed(seed)
        return torch.randn(b, 12, h, w, generator=g) * torch.exp(0.5 * torch.randn(b, 12, 1, 1, generator=g))
    G = lambda s: torch.Generator().manual_seed(s)
    plain = (('fuse_pairs', 0), ('share_s', 0), ('fold_final', 0), ('fold_down', 0), ('fold_lo', 0))
    out = []
    for b, h, w in ((1, 9, 36), (2, 16, 40)):
        tag = '%dx%dx%d' % (b, h, w)
        for c_odd, c_even in ((10, 18), (16, 20)):
            net = pair_net(G(c_even), 12, c_odd, c_even, False)
            out += [('plain_%d_%d_%s' % (c_odd, c_even, tag), net, x(1, b, h, w), plain, (5, 2, 0, 0), ()),
                    ('share_add_%d_%d_%s' % (c_odd, c_even, tag), net, x(1, b, h, w), (('fuse_pairs', 0), ('share_s', 2)), (5, 2, 0, 0), ()),
                    ('pair_%d_%d_%s' % (c_odd, c_even, tag), net, x(1, b, h, w), (('fuse_pairs', 3),), (5, 2, 0, 0), ()),
                    ('pair_merged_%d_%d_%s' % (c_odd, c_even, tag), net, x(1, b, h, w), (('fuse_pairs', 2),), (5, 2, 0, 0), ())]
        out.append(('plain_lead2_' + tag, pair_net(G(3), 12, 10, 18, False, 2), x(2, b, h, w), plain, (5, 2, 0, 0), ()))
        out.append(('tail_' + tag, tail_net(G(4), 10, 18, 5), x(3, b, h, w), (('fuse_pairs', 0), ('share_s', 0), ('fold_final', 2)), (5, 2, 0, 0), ()))
        for r_cout in (40, 33):   # pooled tensor packed at 16 x 40 (20 columns), fp32 at 9 x 36 (18)
            out.append(('down2_%d_%s' % (r_cout, tag), down_net(G(5), 10, 18, r_cout), x(4, b, h, w), (('fuse_pairs', 0), ('share_s', 0), ('fold_down', 2)),
                        (5, 2, 0, 0), (('fold_down', 2),)))
        out.append(('down3_' + tag, down_net(G(6), 16, 46, 96), x(5, b, h, w), (('fuse_pairs', 0), ('share_s', 0), ('fold_down', 2)), (5, 3, 0, 0),
                    (('fold_down', 2),)))
        out.append(('lo_' + tag, lo_net(G(7), 16, 46, 63), x(6, b, 2 * h, 2 * w), (('fuse_pairs', 0), ('share_s', 0), ('fold_lo', 2)), (5, 3, 0, 0),
                    (('fold_lo', 2),)))
        out.append(('block_1x1_pool_res_' + tag, _block_net(G(8), 12), x(7, b, h if h % 2 == 0 else h + 1, w), plain, (5, 2, 0, 0), ()))
        out.append(('slices_1x1_' + tag, slices_net(G(9), 1, 1), x(8, b, h, w), plain, (5, 2, 0, 0), ()))
        out.append(('slices_stride2_' + tag, slices_net(G(10), 3, 2), x(9, b, 2 * h, 2 * w), plain, (5, 2, 0, 0), ()))
        out.append(('slices_fp32_input_' + tag, slices_net(G(11), 3, 1, 'input'), x(10, b, h, w), plain, (5, 2, 0, 0), ()))
        out.append(('pooled_18_' + tag, pooled_net(G(12)), x(11, b, 2 * h, 2 * w), plain, (5, 2, 0, 0), ()))
    return out


def dump():
    import ctypes
    import torch
    from helpers import MiniNet
    from panoptic_forecasting_amd import lib as pflib
    L = pflib.load()
    sha = lambda t: hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:32]
    for name, (spec, P), x, options, force, process in cases():
        for k, v in process:
            pflib.check(L.pf_set_option(k.encode(), v), 'pf_set_option')
        pflib.check(L.pf_debug_force_conv(*force), 'pf_debug_force_conv')
        net = MiniNet(spec, P)
        for k, v in options:
            net.set_option(k, v)
        pflib.profile(True)
        net.run(x.cuda())
        labels = sorted(r['label'].replace('void pf::', '').replace('(pf::ConvArgs)', '') for r in pflib.profile_results())
        pflib.profile(False)
        print('%s status %d kernels %s' % (name, net.status(), ' | '.join(labels)))
        b, h, w = net.bhw
        for t in spec.tensors[1:]:
            off, c, th, tw = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            pflib.check(L.pf_hardnet_tensor_view(net.plan, t.name.encode(), b, h, w, ctypes.byref(off), ctypes.byref(c), ctypes.byref(th),
                                                 ctypes.byref(tw)), 'pf_hardnet_tensor_view')
            n = b * 2 * ((c.value + 3) // 4) * th.value * tw.value * 8      # bytes of the packed form; fp32 NCHW is no longer
            raw = sha(net.ws[off.value:off.value + min(n, net.ws.numel() - off.value)])
            try:
                read = sha(net.tensor(t.name))
            except RuntimeError as e:
                read = 'elided' if 'elided' in str(e) else 'error: %s' % e
            print('%s %s [%d, %d, %d, %d] raw %s fp32 %s' % (name, t.name, b, c.value, th.value, tw.value, raw, read))
        net.close()
        L.pf_debug_force_conv(0, 0, 0, 0)
        for k, _ in process:
            pflib.check(L.pf_set_option(k.encode(), 1), 'pf_set_option')


def dump_train():
    """one training step of helpers.mini_net with its forward on the packed-pair kernels (conv_s4_blocked_kernel): loss and gradient"""
    import torch
    from helpers import MiniTrain, mini_net
    from panoptic_forecasting_amd import lib as pflib
    L = pflib.load()
    sp, g = mini_net(), torch.Generator().manual_seed(17)
    params = {}
    for op in sp.conv_ops():
        pr = {'w': torch.randn(op.cout, op.cin, op.k, op.k, generator=g) * (2.0 / (op.cin * op.k * op.k)) ** 0.5}
        if op.bn:
            pr.update(gamma=torch.rand(op.cout, generator=g) + 0.5, beta=torch.randn(op.cout, generator=g) * 0.2, mean=torch.zeros(op.cout),
                      var=torch.ones(op.cout))
        else:
            pr['b'] = torch.randn(op.cout, generator=g) * 0.1
        params[op.name] = pr
    x = torch.randn(3, 6, 24, 40, generator=g)
    lab = torch.randint(0, 11, (3, 45, 81), generator=g)
    pflib.check(L.pf_set_option(b'train_forward_s4', 1), 'pf_set_option')
    try:
        net = MiniTrain(sp, params)
        pflib.profile(True)
        loss = net.step(x.cuda(), lab.cuda())
        labels = sorted(r['label'].replace('void pf::', '').replace('(pf::ConvArgs)', '') for r in pflib.profile_results() if 'conv_s4' in r['label'])
        pflib.profile(False)
        print('train_24x40 loss %r packed-pair forward convs %d kernels %s' % (loss, net.path_stats()[7], ' | '.join(labels)))
        print('train_24x40 grad %s' % hashlib.sha256(net.grad.cpu().numpy().tobytes()).hexdigest()[:32])
        net.close()
    finally:
        L.pf_set_option(b'train_forward_s4', 0)


def main():
    libs = sys.argv[1:]
    if len(libs) < 2:
        if libs:
            os.environ['PF_LIBPFHIP'] = os.path.abspath(libs[0])
        dump()
        dump_train()
        return 0
    outs = []
    for lib in libs:   # a fresh process per library: the loader maps one
        env = dict(os.environ, PF_LIBPFHIP=os.path.abspath(lib))
        outs.append(subprocess.run([sys.executable, os.path.abspath(__file__), lib], env=env, capture_output=True, text=True, check=True).stdout)
    print(outs[0], end='')
    bad = 0
    for lib, o in zip(libs[1:], outs[1:]):
        same = o == outs[0]
        bad += not same
        print('%s against %s: %s (%d lines)' % (lib, libs[0], 'same' if same else 'DIFFERENT', len(o.splitlines())))
        if not same:
            print('\n'.join(l for l in o.splitlines() if l not in set(outs[0].splitlines())))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
