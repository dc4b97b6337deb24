"""conv_s4 share / add (plan option share_s): a pair P = conv3x3(S), C = conv3x3(P ++ S ++ others) of a HarDBlock as two launches that
read S once.  The share launch replaces P's: its matrix holds P's rows and, from P's couts rounded up to 4 on, C's rows over the columns
of S, whose sums (times C's power-of-two scale; no bias, no ReLU) go to an fp32 scratch tensor.  The add launch replaces C's: it runs
over C's other ranges and forms v = fma(acc, acc_scale, stored) + bias.  Against float64 torch at 2e-5 (1 + max |ref|),
against the two plain launches (share_s = 0) at 1e-5 (1 + max |ref|); which kernels ran is read from the profile labels."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PF_STATUS_RANGE = 1


@pytest.fixture
def force_conv():
    from panoptic_forecasting_amd import lib as pflib
    L = pflib.load()
    yield lambda kind, p0, p1, p2: pflib.check(L.pf_debug_force_conv(kind, p0, p1, p2), 'pf_debug_force_conv')
    L.pf_debug_force_conv(0, 0, 0, 0)


def pair_net(g, cin0, c_odd, c_even, deep, lead=0, c0=24):
    """HarDBlock wiring (hardnet.py:177-194) with free channel counts: L1 = f(t0), L2 = f(L1 ++ t0), L3 = f(L2), L4 = f(L3 ++ L2 ++ t0) and,
    `deep`, L5 = f(L4), L6 = f(L5 ++ L4), L7 = f(L6), L8 = f(L7 ++ L6 ++ L4 ++ t0): odd layers and the last even one are slots of the
    block's output tensor, then a 3x3 conv over it.  `lead` channels of another conv in front of the slots move every offset by `lead`
    (2: every slice starts in the middle of a channel group).  Returns the spec and its parameters."""
    from helpers import MiniSpec
    from panoptic_forecasting_amd import hardnet_arch as arch
    S = arch.Src
    spec = MiniSpec(cin0)
    t0 = spec.conv('t0', [S(0, 0, cin0)], c0, 3)
    n_odd = 4 if deep else 2
    out_ch = lead + n_odd * c_odd + c_even
    out = spec.tensor('out', out_ch)
    shapes = [('t0', cin0, c0)]
    if lead:
        spec.conv('L0', [S(t0, 0, c0)], lead, 3, dst=out, dst_choff=0)
        shapes += [('L0', c0, lead)]
    spec.conv('L1', [S(t0, 0, c0)], c_odd, 3, dst=out, dst_choff=lead)
    l2 = spec.conv('L2', [S(out, lead, c_odd), S(t0, 0, c0)], c_even, 3)
    spec.conv('L3', [S(l2, 0, c_even)], c_odd, 3, dst=out, dst_choff=lead + c_odd)
    shapes += [('L1', c0, c_odd), ('L2', c_odd + c0, c_even), ('L3', c_even, c_odd)]
    if not deep:
        spec.conv('L4', [S(out, lead + c_odd, c_odd), S(l2, 0, c_even), S(t0, 0, c0)], c_even, 3, dst=out, dst_choff=lead + 2 * c_odd)
        shapes += [('L4', c_odd + c_even + c0, c_even)]
    else:
        l4 = spec.conv('L4', [S(out, lead + c_odd, c_odd), S(l2, 0, c_even), S(t0, 0, c0)], c_even, 3)
        spec.conv('L5', [S(l4, 0, c_even)], c_odd, 3, dst=out, dst_choff=lead + 2 * c_odd)
        l6 = spec.conv('L6', [S(out, lead + 2 * c_odd, c_odd), S(l4, 0, c_even)], c_even, 3)
        spec.conv('L7', [S(l6, 0, c_even)], c_odd, 3, dst=out, dst_choff=lead + 3 * c_odd)
        spec.conv('L8', [S(out, lead + 3 * c_odd, c_odd), S(l6, 0, c_even), S(l4, 0, c_even), S(t0, 0, c0)], c_even, 3, dst=out,
                  dst_choff=lead + 4 * c_odd)
        shapes += [('L4', c_odd + c_even + c0, c_even), ('L5', c_even, c_odd), ('L6', c_odd + c_even, c_even), ('L7', c_even, c_odd),
                   ('L8', c_odd + 2 * c_even + c0, c_even)]
    spec.conv('fin', [S(out, 0, out_ch)], 9, 3, relu=False)
    shapes += [('fin', out_ch, 9)]
    P = {n: (torch.randn(co, ci, 3, 3, generator=g) / (ci * 9) ** 0.5, torch.randn(co, generator=g) * 0.5) for n, ci, co in shapes}
    return spec, P


def pair_ref(x, P, deep, lead=0):
    D = {k: (v[0].double(), v[1].double()) for k, v in P.items()}
    cv = lambda n, t: F.relu(F.conv2d(t, *D[n], padding=1))
    t0 = cv('t0', x.double())
    l1 = cv('L1', t0)
    l2 = cv('L2', torch.cat([l1, t0], 1))
    l3 = cv('L3', l2)
    l4 = cv('L4', torch.cat([l3, l2, t0], 1))
    slots = [cv('L0', t0)] if lead else []
    if not deep:
        out = torch.cat(slots + [l1, l3, l4], 1)
        return {'L2': l2, 'out': out, 'fin': F.conv2d(out, *D['fin'], padding=1)}
    l5 = cv('L5', l4)
    l6 = cv('L6', torch.cat([l5, l4], 1))
    l7 = cv('L7', l6)
    l8 = cv('L8', torch.cat([l7, l6, l4, t0], 1))
    out = torch.cat(slots + [l1, l3, l5, l7, l8], 1)
    return {'L2': l2, 'L4': l4, 'L6': l6, 'out': out, 'fin': F.conv2d(out, *D['fin'], padding=1)}


def run_labels(net, x):
    from panoptic_forecasting_amd import lib as pflib
    pflib.profile(True)
    net.run(x.cuda())
    labels = [r['label'] for r in pflib.profile_results()]
    pflib.profile(False)
    return labels


def check_pair(c_odd, c_even, deep, h, w, b, lead=0):
    """share_s = 2 against float64 and against share_s = 0; returns the labels of the share_s = 2 run"""
    from helpers import MiniNet
    g = torch.Generator().manual_seed(h * 7 + w + c_even + lead)
    x = torch.randn(b, 12, h, w, generator=g) * torch.exp(0.5 * torch.randn(b, 12, 1, 1, generator=g))
    spec, P = pair_net(g, 12, c_odd, c_even, deep, lead)
    ref = pair_ref(x, P, deep, lead)
    got, labels = {}, {}
    for mode in (0, 2):
        net = MiniNet(spec, P).set_option('share_s', mode).set_option('fuse_pairs', 0)
        labels[mode] = run_labels(net, x)
        got[mode] = {k: net.tensor(k).cpu() for k in ref}
        assert net.status() == 0
        net.close()
    assert not any('share' in l or 'add_kernel' in l for l in labels[0]), labels[0]
    for name, r in ref.items():
        r = r.float()
        m = r.abs().max().item()
        e0, e2 = ((got[k][name] - r).abs().max().item() for k in (0, 2))
        d = (got[0][name] - got[2][name]).abs().max().item()
        print('%s: max|ref| %.3g  err two launches %.3g  err share/add %.3g (bar %.3g)  between them %.3g (bar %.3g)' %
              (name, m, e0, e2, 2e-5 * (1 + m), d, 1e-5 * (1 + m)))
    for name, r in ref.items():
        r = r.float()
        m = r.abs().max().item()
        assert (got[2][name] - r).abs().max().item() <= 2e-5 * (1.0 + m), name
        assert (got[0][name] - got[2][name]).abs().max().item() <= 1e-5 * (1.0 + m), name
    return labels[2]


def n_launches(labels, what):
    return sum(what in l for l in labels)


# (P couts, C couts): packed rows = roundup4(P) + C -> 12 + 18 = 30 rows in two tiles, 12 + 20 = exactly 32, 20 + 30 = 50 in four,
# 8 + 10 = 18 in two.  8 x 32: one pixel tile; 9 x 36: partial tiles in both directions, zero padding on every edge; 17 x 40: three
# tile rows, two columns.  9 x 33: the packed-pair kernels take widths that are multiples of 4 only, the plan keeps such a network on
# its fp32-source kernels whatever share_s says - the same results are asked of it
@pytest.mark.parametrize('c_odd,c_even', [(10, 18), (12, 20), (18, 30), (6, 10)])
@pytest.mark.parametrize('h,w,b,deep', [(8, 32, 1, False), (9, 33, 1, False), (9, 36, 2, True), (17, 40, 1, True), (17, 40, 2, False)])
def test_share_add_vs_float64_and_two_launches(c_odd, c_even, h, w, b, deep, force_conv):
    """Every pair of the block runs as share + add (one label per kernel shape), blocks of 4 and 8 layers (C with two to four ranges);
    (10, 18) without `deep`: C's slice of the block output ends on a half group (20 + 18 = 38 channels)."""
    force_conv(5, 2, 0, 0)
    labels = check_pair(c_odd, c_even, deep, h, w, b)
    assert not any('conv_pair_kernel' in l for l in labels), labels
    if w % 4:
        assert not any('conv_s4' in l for l in labels), labels
        return
    assert n_launches(labels, 'conv_s4_share_kernel') >= 1 and n_launches(labels, 'conv_s4_add_kernel') >= 1, labels
    tiles = ((c_odd + 3) // 4 * 4 + c_even + 15) // 16
    assert any('conv_s4_share_kernel<%d, 32, 8, 1>' % (tiles if tiles <= 3 else 2) in l for l in labels), labels
    assert any('conv_s4_add_kernel<2, 32, 8, 1>' in l for l in labels) == (c_even > 16), labels


@pytest.mark.parametrize('c_odd,c_even,nt', [(4, 10, 1), (12, 36, 3)])
def test_share_add_one_and_three_tiles(c_odd, c_even, nt, force_conv):
    """the forms built for one (4 + 10 = 14 rows) and three (12 + 36 = 48 rows) cout tiles per workgroup"""
    force_conv(5, nt, 0, 0)
    labels = check_pair(c_odd, c_even, False, 9, 36, 2)
    assert any('conv_s4_share_kernel<%d, 32, 8, 1>' % nt in l for l in labels), labels
    assert any('conv_s4_add_kernel<%d, 32, 8, 1>' % nt in l for l in labels), labels


def test_share_add_slices_that_start_in_the_middle_of_a_group(force_conv):
    """two channels of another layer in front of the block's slots: P's and C's slices start at channels 2, 12, 22 (the `mis` stores)"""
    force_conv(5, 2, 0, 0)
    labels = check_pair(10, 18, False, 9, 36, 2, lead=2)
    assert n_launches(labels, 'conv_s4_share_kernel') >= 1 and n_launches(labels, 'conv_s4_add_kernel') >= 1, labels


def test_rule_keeps_pairs_whose_rows_do_not_pack_on_two_launches(force_conv):
    """share_s = 1: (16, 28) needs 16 + 28 = 44 rows = three tiles, as many as the two launches have: they stay"""
    from helpers import MiniNet
    force_conv(5, 2, 0, 0)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 12, 9, 36, generator=g)
    spec, P = pair_net(g, 12, 16, 28, False)
    ref = pair_ref(x, P, False)
    net = MiniNet(spec, P).set_option('share_s', 1).set_option('fuse_pairs', 0)
    labels = run_labels(net, x)
    assert not any('share' in l or 'add_kernel' in l for l in labels), labels
    assert n_launches(labels, 'conv_s4_kernel') >= 1
    assert net.status() == 0
    r = ref['fin'].float()
    assert (net.tensor('fin').cpu() - r).abs().max().item() <= 2e-5 * (1.0 + r.abs().max().item())
    net.close()


def _range_net(bias):
    """L1 = t0's first ten channels, L2 = 1000 t0[0] - 1000 L1[0] + bias in every channel: C's sums over S alone reach 1e5"""
    g = torch.Generator().manual_seed(1)
    spec, P = pair_net(g, 12, 10, 18, False)
    P = {k: (torch.zeros_like(w), torch.zeros_like(b)) for k, (w, b) in P.items()}
    for c in range(24):
        P['t0'][0][c, c % 12, 1, 1] = 1.0
    for c in range(10):
        P['L1'][0][c, c, 1, 1] = 1.0
    P['L2'][0][:, 0, 1, 1] = -1000.0     # P's channel 0
    P['L2'][0][:, 10, 1, 1] = 1000.0     # S's channel 0
    P['L2'][1][:] = bias
    return spec, P


@pytest.fixture
def raw_ranges():
    """plans created without the per-channel power-of-two scaling: stored values are the network's own"""
    from panoptic_forecasting_amd import lib as pflib
    L = pflib.load()
    pflib.check(L.pf_set_option(b'normalize_ranges', 0), 'pf_set_option')
    yield
    pflib.check(L.pf_set_option(b'normalize_ranges', 1), 'pf_set_option')


@pytest.mark.parametrize('bias,flag', [(1.0, 0), (1e5, PF_STATUS_RANGE)])
def test_range_guard_sees_final_values_only(bias, flag, force_conv, raw_ranges):
    """the stored sums over S are no tensor's values: 1e5 there with final values of 1 raises nothing; final values of 1e5 raise
    PF_STATUS_RANGE as from the plain kernel"""
    from helpers import MiniNet
    force_conv(5, 2, 0, 0)
    spec, P = _range_net(bias)
    x = torch.full((1, 12, 9, 36), 100.0)
    for mode in (0, 2):
        net = MiniNet(spec, P).set_option('share_s', mode).set_option('fuse_pairs', 0)
        labels = run_labels(net, x)
        assert (n_launches(labels, 'conv_s4_share_kernel') >= 1) == (mode == 2), labels
        assert net.status() & PF_STATUS_RANGE == flag, (mode, net.status())
        if not flag:
            assert net.status() == 0
            l2 = net.tensor('L2').cpu()
            assert (l2 - bias).abs().max().item() <= 1e5 * 2.0 ** -20, (l2 - bias).abs().max().item()   # two operands of 1e5 at 2^-22 each
        net.close()


def test_captured_forward_replays_equal_eager(force_conv):
    """one captured forward of a (10, 18) block, replayed five times: the same bits as the eager forward every time"""
    from helpers import MiniNet
    from panoptic_forecasting_amd import lib as pflib
    L = pflib.load()
    force_conv(5, 2, 0, 0)
    g = torch.Generator().manual_seed(11)
    b, h, w = 2, 17, 40
    x = torch.randn(b, 12, h, w, generator=g).cuda()
    spec, P = pair_net(g, 12, 10, 18, True)
    net = MiniNet(spec, P).set_option('share_s', 2).set_option('fuse_pairs', 0)
    labels = run_labels(net, x)
    assert n_launches(labels, 'conv_s4_share_kernel') >= 1 and n_launches(labels, 'conv_s4_add_kernel') >= 1, labels
    names = ('L2', 'L4', 'L6', 'out', 'fin')
    want = {k: net.tensor(k).clone() for k in names}

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
    for rep in range(5):
        net.ws[2048:].zero_()          # (behind the status block) a replay that skipped its work would leave zeros
        graph.replay()
        torch.cuda.synchronize()
        for k in names:
            assert torch.equal(net.tensor(k), want[k]), (rep, k)
        assert net.status() == 0
    net.close()
