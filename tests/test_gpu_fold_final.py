"""conv_s4 tail (plan option fold_final): the last 3x3 layer L4 of a HarDBlock whose slice of the block's output has one reader, a 1x1
conv `fin` without ReLU into fp32, runs as ONE launch: L4's finished values stay in registers as the fp16 pair `fin` would read back and
are multiplied by fin's weights behind the centre pixels of fin's other channels (the L1 and L3 slices); fin's output is stored, L4's
slice is not, fin's launch goes away.  fold_final = 2 against float64 torch at 2e-5 (1 + max |ref|) and against the two
plain launches (fold_final = 0) at 1e-5 (1 + max |ref|) - the bars tests/test_gpu_share_s.py holds the share / add launches to: the same
products, another grouping of the fp32 sum.  Which kernels ran is read from the profile labels.

With the fold on the block's output tensor cannot be tapped (its last slice does not exist), so its L1 / L3 slices are compared as the
bytes of their packed planes in the workspace, fold on against fold off (the same launches wrote them: equal bits), and against float64
through the fold_final = 0 run and through the tensors that read them (L2, fin).

The packed-pair kernels take widths that are multiples of 4 only: at 9 x 33 the plan keeps the whole network on its fp32-source kernels
whatever fold_final says - the same results are asked of it - and 9 x 36 is the folded case with partial tiles in both directions."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from test_fold_final_host import tail_net

pytestmark = pytest.mark.gpu

PF_STATUS_RANGE = 1
TAIL = 'conv_s4_tail_kernel<2, 32, 8, 1>'


@pytest.fixture
def force_conv():
    from panoptic_forecasting_amd import lib as pflib
    L = pflib.load()
    yield lambda kind, p0, p1, p2: pflib.check(L.pf_debug_force_conv(kind, p0, p1, p2), 'pf_debug_force_conv')
    L.pf_debug_force_conv(0, 0, 0, 0)


@pytest.fixture
def raw_ranges():
    """plans created without the per-channel power-of-two scaling: stored values are the network's own"""
    from panoptic_forecasting_amd import lib as pflib
    L = pflib.load()
    pflib.check(L.pf_set_option(b'normalize_ranges', 0), 'pf_set_option')
    yield
    pflib.check(L.pf_set_option(b'normalize_ranges', 1), 'pf_set_option')


def tail_ref(x, P, lead=0, fin_relu=False):
    D = {k: (v[0].double(), v[1].double()) for k, v in P.items()}
    cv = lambda n, t: F.relu(F.conv2d(t, *D[n], padding=1))
    t0 = cv('t0', x.double())
    l1 = cv('L1', t0)
    l2 = cv('L2', torch.cat([l1, t0], 1))
    l3 = cv('L3', l2)
    l4 = cv('L4', torch.cat([l3, l2, t0], 1))
    out = torch.cat(([cv('L0', t0)] if lead else []) + [l1, l3, l4], 1)
    fin = F.conv2d(out, *D['fin'])
    ref = {'L2': l2, 'out': out, 'fin': F.relu(fin) if fin_relu else fin}
    if 'side' in D:
        ref['side'] = F.conv2d(out, *D['side'])
    return ref


def run_labels(net, x):
    from panoptic_forecasting_amd import lib as pflib
    pflib.profile(True)
    net.run(x.cuda())
    labels = sorted(r['label'] for r in pflib.profile_results() for _ in range(r['launches']))   # one entry per launch
    pflib.profile(False)
    return labels


def slot_planes(net, name, groups):
    """both terms of the first `groups` channel groups of a packed tensor as the last forward left them in the workspace"""
    from panoptic_forecasting_amd import lib as pflib
    b, h, w = net.bhw
    off, c, th, tw = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    pflib.check(pflib.load().pf_hardnet_tensor_view(net.plan, name.encode(), b, h, w, ctypes.byref(off), ctypes.byref(c), ctypes.byref(th),
                                                    ctypes.byref(tw)), 'pf_hardnet_tensor_view')
    c4 = (c.value + 3) // 4
    raw = net.ws[off.value:off.value + b * 2 * c4 * th.value * tw.value * 8].view(torch.int16).view(b, 2, c4, th.value, tw.value, 4)
    return raw[:, :, :groups].cpu(), raw[:, :, groups:].cpu()


def assert_fold_close(ref, two, fold):
    """every tensor of the float64 reference: the two launches and the fold within 2e-5 (1 + max |ref|) of it, within 1e-5 (1 + max |ref|)
    of each other; a tensor the fold run could not tap (elided) is missing from `fold`.  Prints the figures first"""
    for name, r in ref.items():
        r = r.float()
        m = r.abs().max().item()
        e0 = (two[name] - r).abs().max().item()
        e2 = (fold[name] - r).abs().max().item() if name in fold else float('nan')
        d = (two[name] - fold[name]).abs().max().item() if name in fold else float('nan')
        print('%s: max|ref| %.3g  err two launches %.3g  err fold %.3g (bar %.3g)  between them %.3g (bar %.3g)' %
              (name, m, e0, e2, 2e-5 * (1 + m), d, 1e-5 * (1 + m)))
    for name, r in ref.items():
        r = r.float()
        m = r.abs().max().item()
        assert two[name].shape == r.shape
        assert (two[name] - r).abs().max().item() <= 2e-5 * (1.0 + m), name
        if name in fold:
            assert fold[name].shape == r.shape
            assert (fold[name] - r).abs().max().item() <= 2e-5 * (1.0 + m), name
            assert (two[name] - fold[name]).abs().max().item() <= 1e-5 * (1.0 + m), name


def check_tail(c_odd, c_even, fin_cout, h, w, b, folded, options=(), **kw):
    """fold_final = 2 against float64 and against fold_final = 0; `folded`: the tail launch must have run (else the two plain ones).
    Returns the labels of the fold_final = 2 run"""
    from helpers import MiniNet
    g = torch.Generator().manual_seed(h * 7 + w + c_even + fin_cout)
    x = torch.randn(b, 12, h, w, generator=g) * torch.exp(0.5 * torch.randn(b, 12, 1, 1, generator=g))
    spec, P = tail_net(g, c_odd, c_even, fin_cout, **kw)
    ref = tail_ref(x, P, kw.get('lead', 0), kw.get('fin_relu', False))
    got, labels, planes = {}, {}, {}
    front_groups = (kw.get('lead', 0) + 2 * c_odd) // 4
    for mode in (0, 2):
        net = MiniNet(spec, P).set_option('fold_final', mode).set_option('fuse_pairs', 0).set_option('share_s', 0)
        for name, value in options:
            net.set_option(name, value)
        labels[mode] = run_labels(net, x)
        ran = any('conv_s4_tail_kernel' in l for l in labels[mode])
        assert ran == (folded and mode == 2), labels[mode]
        assert net.status() == 0
        names = [k for k in ref if not (ran and k == 'out')]
        got[mode] = {k: net.tensor(k).cpu() for k in names}
        if ran:
            with pytest.raises(RuntimeError, match='elided'):       # the tap check
                net.tensor('out')
        if folded:
            planes[mode] = slot_planes(net, 'out', front_groups)
        net.close()
    if folded:
        assert sum(TAIL in l for l in labels[2]) == 1 and not any('conv_s4_1x1_kernel' in l for l in labels[2]), labels[2]
        assert sum('conv_s4_kernel' in l for l in labels[0]) == sum('conv_s4_kernel' in l for l in labels[2]) + 1, (labels[0], labels[2])
        assert torch.equal(planes[0][0], planes[2][0])               # the L1 / L3 slices: the same bits
        assert planes[0][1].any() and not planes[2][1].any()         # L4's slice: stored by the plain launch, never by the tail launch
    else:
        assert any('conv_s4_1x1_kernel' in l for l in labels[2]) == (w % 4 == 0), labels[2]
        assert labels[0] == labels[2]
    assert_fold_close(ref, got[0], got[2])
    return labels[2]


# (c_odd, c_even, fin couts) at h x w, batch b.  (10, 28, 11) = FC-HarDNet-70's last block: 16 x 40: a partial tile in x, two tile rows;
# 9 x 36: partial tiles in both directions, a last tile of four columns, an odd height.  (10, 18, 5): 14 zero rows in L4's second cout
# tile, fewer than 8 logits, the block output ends on a half group.  (12, 32, 16): full tiles, a full logit tile.  (16, 20, 1): 32
# channels in front of the slice (every K position of the chunk from memory in use), one logit
@pytest.mark.parametrize('c_odd,c_even,fin_cout,h,w,b', [(10, 28, 11, 16, 40, 2), (10, 28, 11, 9, 36, 1), (10, 18, 5, 16, 32, 1),
                                                         (12, 32, 16, 8, 64, 1), (16, 20, 1, 9, 36, 2)])
def test_fold_vs_float64_and_two_launches(c_odd, c_even, fin_cout, h, w, b, force_conv):
    force_conv(5, 2, 0, 0)
    check_tail(c_odd, c_even, fin_cout, h, w, b, True)


@pytest.mark.parametrize('c0', [32, 40])
def test_fold_behind_more_than_four_rounds(c0, force_conv):
    """a block input of 32 / 40 channels: L4 runs 9 / 10 rounds, its last group of four collected-tap rounds is a partial one"""
    force_conv(5, 2, 0, 0)
    check_tail(10, 28, 11, 16, 40, 1, True, c0=c0)


def test_width_that_is_no_multiple_of_four_runs_no_packed_pair_kernel(force_conv):
    """9 x 33: odd sizes; the network stays on its fp32-source kernels, the same results are asked of it"""
    force_conv(5, 2, 0, 0)
    labels = check_tail(10, 28, 11, 9, 33, 1, False)
    assert not any('conv_s4' in l for l in labels), labels


@pytest.mark.parametrize('kw', [dict(lead=2), dict(second_reader=True), dict(fin_relu=True), dict(fin_cout=17)],
                         ids=['slice_in_mid_group', 'second_reader', 'fin_relu', 'fin_17_couts'])
def test_tables_that_fall_back_to_two_launches(kw, force_conv):
    force_conv(5, 2, 0, 0)
    args = dict(c_odd=10, c_even=28, fin_cout=11)
    args.update(kw)
    labels = check_tail(args.pop('c_odd'), args.pop('c_even'), args.pop('fin_cout'), 9, 36, 2, False, **args)
    assert any('conv_s4_kernel<2, 32, 8, 1>' in l for l in labels), labels


def test_k_split_shape_falls_back(force_conv):
    """8 x 32 tiles with two wave groups splitting L4's 8 rounds: the form is built without a K split"""
    force_conv(5, 2, 3, 0)
    labels = check_tail(10, 28, 11, 9, 36, 2, False)
    assert any('conv_s4_kernel<2, 32, 8, 2>' in l for l in labels), labels


def test_add_launch_of_a_share_pair_falls_back(force_conv):
    """share_s = 2: L4 runs as the add launch of the pair (L3, L4)"""
    force_conv(5, 2, 0, 0)
    labels = check_tail(10, 28, 11, 9, 36, 2, False, options=(('share_s', 2),))
    assert any('conv_s4_add_kernel' in l for l in labels), labels


def test_rule_leaves_small_launches_alone(force_conv):
    """fold_final = 1 (the default): launches of a class nobody measured stay two launches and the block's output can be tapped"""
    from helpers import MiniNet
    force_conv(5, 2, 0, 0)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 12, 9, 36, generator=g)
    spec, P = tail_net(g, 10, 28, 11)
    ref = tail_ref(x, P)
    net = MiniNet(spec, P).set_option('fuse_pairs', 0)
    labels = run_labels(net, x)
    assert not any('tail' in l for l in labels) and any('conv_s4_1x1_kernel' in l for l in labels), labels
    assert net.status() == 0
    for k in ('out', 'fin'):
        r = ref[k].float()
        assert (net.tensor(k).cpu() - r).abs().max().item() <= 2e-5 * (1.0 + r.abs().max().item())
    net.close()


def test_range_guard_sees_the_elided_values(force_conv, raw_ranges):
    """L4's weights and bias times 2^17: the values its slice would hold exceed 65504; PF_STATUS_RANGE with the fold on as with it off"""
    from helpers import MiniNet
    force_conv(5, 2, 0, 0)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(1, 12, 9, 36, generator=g)
    spec, P = tail_net(g, 10, 28, 11)
    P['L4'] = (P['L4'][0] * 2.0 ** 17, P['L4'][1] * 2.0 ** 17)
    assert tail_ref(x, P)['out'].max().item() > 65504.0
    for mode in (0, 2):
        net = MiniNet(spec, P).set_option('fold_final', mode).set_option('fuse_pairs', 0).set_option('share_s', 0)
        labels = run_labels(net, x)
        assert any('conv_s4_tail_kernel' in l for l in labels) == (mode == 2), labels
        assert net.status() & PF_STATUS_RANGE == PF_STATUS_RANGE, (mode, net.status())
        net.close()


def test_captured_forward_replays_equal_eager(force_conv):
    """one captured forward with the tail launch, replayed three times: the same bits as the eager forward every time"""
    from helpers import MiniNet
    from panoptic_forecasting_amd import lib as pflib
    L = pflib.load()
    force_conv(5, 2, 0, 0)
    g = torch.Generator().manual_seed(11)
    b, h, w = 2, 16, 40
    x = torch.randn(b, 12, h, w, generator=g).cuda()
    spec, P = tail_net(g, 10, 28, 11)
    net = MiniNet(spec, P).set_option('fold_final', 2).set_option('fuse_pairs', 0).set_option('share_s', 0)
    labels = run_labels(net, x)
    assert sum(TAIL in l for l in labels) == 1, labels
    want = {k: net.tensor(k).clone() for k in ('L2', 'fin')}

    def enqueue():
        pflib.check(L.pf_hardnet_forward_dense(net.plan, x.data_ptr(), b, h, w, 0, 0, None, 0, None, None, net.ws.data_ptr(), net.ws.numel(),
                                               pflib.stream_ptr()), 'pf_hardnet_forward_dense')

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enqueue()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue()
    for rep in range(3):
        net.ws[2048:].zero_()          # (behind the status block) a replay that skipped its work would leave zeros
        graph.replay()
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(net.tensor(k), want[k]), (rep, k)
        assert net.status() == 0
    net.close()
