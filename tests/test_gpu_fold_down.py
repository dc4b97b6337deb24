"""conv_s4 down (plan option fold_down): the last 3x3 layer L4 of a HarDBlock in front of the block's transition - a 1x1 conv `dn` with
ReLU over the block's output and its 2x2 average pool `pl` - runs as ONE launch: L4's finished values are stored as ever and, still in
registers as the fp16 pair `dn` would read back, are multiplied by dn's weights behind the centre pixels of dn's other channels (the L1
and L3 slices); the pooled output is stored, dn's launch goes away.  fold_down = 2 against float64 torch at
2e-5 (1 + max |ref|) and against the two launches (fold_down = 0) at 1e-5 (1 + max |ref|) - the bars of tests/test_gpu_fold_final.py and
tests/test_gpu_share_s.py: the same products, another grouping of the fp32 sum.  L4's slice - the whole block output - holds the same
bits in both modes.  Which kernels ran is read from the profile labels.

The pooled tensor is stored as packed pairs where the conv behind it reads packed pairs (pooled widths that are multiples of 4: 20, 16,
32) and as fp32 NCHW otherwise (18): the launch has both stores, as dn's own launch has."""
import pytest
import torch
import torch.nn.functional as F

from test_fold_down_host import both_net, down_net
from test_gpu_fold_final import TAIL, assert_fold_close, force_conv, raw_ranges, run_labels, slot_planes, tail_ref  # noqa: F401

pytestmark = pytest.mark.gpu

PF_STATUS_RANGE = 1
DOWN = 'conv_s4_down_kernel<2, 32, 8, 1>'


@pytest.fixture
def packs_down():
    """plans are created with the down form's fragments packed whatever the process-wide value was, and mode 2 is what they start with"""
    from panoptic_forecasting_amd import lib as pflib
    L = pflib.load()
    pflib.check(L.pf_set_option(b'fold_down', 2), 'pf_set_option')
    yield
    pflib.check(L.pf_set_option(b'fold_down', 1), 'pf_set_option')


def down_ref(x, P, lead=0, r_relu=True, pool=True):
    D = {k: (v[0].double(), v[1].double()) for k, v in P.items()}
    cv = lambda n, t: F.relu(F.conv2d(t, *D[n], padding=1))
    t0 = cv('t0', x.double())
    l1 = cv('L1', t0)
    l2 = cv('L2', torch.cat([l1, t0], 1))
    l3 = cv('L3', l2)
    l4 = cv('L4', torch.cat([l3, l2, t0], 1))
    out = torch.cat(([cv('L0', t0)] if lead else []) + [l1, l3, l4], 1)
    dn = F.conv2d(out, *D['dn'])
    dn = F.relu(dn) if r_relu else dn
    ref = {'L2': l2, 'out': out}
    ref['pl' if pool else 'dn'] = F.avg_pool2d(dn, 2) if pool else dn
    if 'sk' in D:
        ref['sk'] = F.conv2d(out, *D['sk'])
    return ref


def make_net(spec, P, mode, options=()):
    from helpers import MiniNet
    net = MiniNet(spec, P).set_option('fold_down', mode).set_option('fuse_pairs', 0).set_option('share_s', 0)
    for name, value in options:
        net.set_option(name, value)
    return net


def check_down(c_odd, c_even, r_cout, h, w, b, folded, options=(), **kw):
    """fold_down = 2 against float64 and against fold_down = 0; `folded`: the down launch must have run (else the two launches).  Returns
    the labels of the fold_down = 2 run"""
    g = torch.Generator().manual_seed(h * 7 + w + c_even + r_cout)
    x = torch.randn(b, 12, h, w, generator=g) * torch.exp(0.5 * torch.randn(b, 12, 1, 1, generator=g))
    spec, P = down_net(g, c_odd, c_even, r_cout, **kw)
    ref = down_ref(x, P, kw.get('lead', 0), kw.get('r_relu', True), kw.get('pool', True))
    got, labels, planes = {}, {}, {}
    for mode in (0, 2):
        net = make_net(spec, P, mode, options)
        labels[mode] = run_labels(net, x)
        ran = any('conv_s4_down_kernel' in l for l in labels[mode])
        assert ran == (folded and mode == 2), labels[mode]
        assert net.status() == 0
        got[mode] = {k: net.tensor(k).cpu() for k in ref}
        planes[mode] = slot_planes(net, 'out', 0)[1]       # the block output as stored: every group, both terms
        net.close()
    if folded:
        assert sum(DOWN in l for l in labels[2]) == 1 and not any('+pool' in l for l in labels[2]), labels[2]
        assert sum('+pool' in l and 'conv_s4_1x1_kernel' in l for l in labels[0]) == 1, labels[0]
        assert sum('conv_s4_kernel' in l for l in labels[0]) == sum('conv_s4_kernel' in l for l in labels[2]) + 1, (labels[0], labels[2])
        assert len(labels[0]) == len(labels[2]) + 1
    else:
        assert labels[0] == labels[2]
    assert planes[0].any() and torch.equal(planes[0], planes[2])      # L4's slice (and L1's, L3's): the same bits
    assert_fold_close(ref, got[0], got[2])
    return labels[2]


# (c_odd, c_even, dn couts) at h x w, batch b.  (10, 28, 64) = FC-HarDNet-70's first block and transition: 16 x 40: a partial tile in x,
# two tile rows; 9 x 36: an odd height (the pool drops the last row), a last tile of four columns.  (10, 18, 40): 14 zero rows in L4's
# second cout tile, dn's last cout tile half full.  (12, 32, 16): one tile of dn.  (16, 20, 33) at 10 x 36: 32 channels in front of the
# slice (every K position of the chunk from memory in use), dn's third tile holds one cout; at 16 x 40 the same into packed pairs: the
# pooled tensor ends in the middle of a group
@pytest.mark.parametrize('c_odd,c_even,r_cout,h,w,b', [(10, 28, 64, 16, 40, 2), (10, 28, 64, 9, 36, 1), (10, 18, 40, 16, 32, 1),
                                                       (12, 32, 16, 8, 64, 1), (16, 20, 33, 10, 36, 2), (16, 20, 33, 16, 40, 1)])
def test_fold_vs_float64_and_two_launches(c_odd, c_even, r_cout, h, w, b, force_conv, packs_down):
    force_conv(5, 2, 0, 0)
    check_down(c_odd, c_even, r_cout, h, w, b, True)


def test_both_forms_in_one_plan(force_conv, packs_down):
    """a down block (10, 28, 64) and, behind its pool at 8 x 20, a tail block (10, 28, 11): the schedule's fold pass runs once per form over
    the same step list.  One launch of each form, neither 1x1 conv on its own; the bars of check_down / check_tail against float64 and
    against the same net with both options 0"""
    force_conv(5, 2, 0, 0)
    g = torch.Generator().manual_seed(21)
    x = torch.randn(1, 12, 16, 40, generator=g) * torch.exp(0.5 * torch.randn(1, 12, 1, 1, generator=g))
    spec, P = both_net(g)
    ref = down_ref(x, P)
    up = tail_ref(ref['pl'], dict({k[2:]: v for k, v in P.items() if k.startswith('u.')}, fin=P['fin']))
    ref.update({'u.L2': up['L2'], 'u.out': up['out'], 'fin': up['fin']})
    got, labels = {}, {}
    for mode in (0, 2):
        net = make_net(spec, P, mode, (('fold_final', mode),))
        labels[mode] = run_labels(net, x)
        assert net.status() == 0
        got[mode] = {k: net.tensor(k).cpu() for k in ref if not (mode == 2 and k == 'u.out')}   # (its last slice is elided)
        net.close()
    assert sum(DOWN in l for l in labels[2]) == 1 and sum('conv_s4_down_kernel' in l for l in labels[2]) == 1, labels[2]
    assert sum(TAIL in l for l in labels[2]) == 1 and sum('conv_s4_tail_kernel' in l for l in labels[2]) == 1, labels[2]
    assert not any('conv_s4_1x1_kernel' in l for l in labels[2]), labels[2]        # dn (+pool) and fin run in no launch of their own ...
    assert sum('conv_s4_1x1_kernel' in l for l in labels[0]) == 2 and not any('tail' in l or 'down' in l for l in labels[0]), labels[0]
    assert len(labels[0]) == len(labels[2]) + 2                                      # ... as they do with the folds off
    assert_fold_close(ref, got[0], got[2])


def test_second_reader_of_the_block_output_reads_what_the_fold_stored(force_conv, packs_down):
    """`sk`, a 1x1 conv over the block's output behind the pool (the decoder's skip connection), with the fold on"""
    force_conv(5, 2, 0, 0)
    check_down(10, 28, 64, 16, 40, 2, True, skip=True)


@pytest.mark.parametrize('kw', [dict(r_cout=65), dict(pool=False)], ids=['dn_65_couts', 'no_pool'])
def test_tables_that_fall_back_to_two_launches(kw, force_conv, packs_down):
    force_conv(5, 2, 0, 0)
    args = dict(c_odd=10, c_even=28, r_cout=64)
    args.update(kw)
    labels = check_down(args.pop('c_odd'), args.pop('c_even'), args.pop('r_cout'), 16, 40, 2, False, **args)
    assert any('conv_s4_kernel<2, 32, 8, 1>' in l for l in labels), labels


def test_k_split_shape_falls_back(force_conv, packs_down):
    """8 x 32 tiles with two wave groups splitting L4's 8 rounds: the form is built without a K split"""
    force_conv(5, 2, 3, 0)
    labels = check_down(10, 28, 64, 16, 40, 2, False)
    assert any('conv_s4_kernel<2, 32, 8, 2>' in l for l in labels), labels


def test_add_launch_of_a_share_pair_falls_back(force_conv, packs_down):
    """share_s = 2: L4 runs as the add launch of the pair (L3, L4)"""
    force_conv(5, 2, 0, 0)
    labels = check_down(10, 28, 64, 16, 40, 2, False, options=(('share_s', 2),))
    assert any('conv_s4_add_kernel' in l for l in labels), labels


def test_rule_leaves_small_launches_alone(force_conv, packs_down):
    """fold_down = 1: launches of a class nobody measured stay two launches"""
    force_conv(5, 2, 0, 0)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 12, 16, 40, generator=g)
    spec, P = down_net(g, 10, 28, 64)
    ref = down_ref(x, P)
    net = make_net(spec, P, 1)
    labels = run_labels(net, x)
    assert not any('down' in l for l in labels) and sum('+pool' in l for l in labels) == 1, labels
    assert net.status() == 0
    for k in ('out', 'pl'):
        r = ref[k].float()
        assert (net.tensor(k).cpu() - r).abs().max().item() <= 2e-5 * (1.0 + r.abs().max().item())
    net.close()


@pytest.mark.parametrize('layer', ['L4', 'dn'])
def test_range_guard_sees_both_stored_tensors(layer, force_conv, raw_ranges, packs_down):
    """L4's weights and bias times 2^17: its slice exceeds 65504.  dn's: the slice is in range, the pooled values are not.
    PF_STATUS_RANGE with the fold on as with it off"""
    force_conv(5, 2, 0, 0)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(1, 12, 16, 40, generator=g)
    spec, P = down_net(g, 10, 28, 64)
    P[layer] = (P[layer][0] * 2.0 ** 17, P[layer][1] * 2.0 ** 17)
    ref = down_ref(x, P)
    if layer == 'L4':
        assert ref['out'].max().item() > 65504.0
    else:
        assert ref['out'].max().item() < 65504.0 / 64 and ref['pl'].max().item() > 65504.0
    for mode in (0, 2):
        net = make_net(spec, P, mode)
        labels = run_labels(net, x)
        assert any('conv_s4_down_kernel' in l for l in labels) == (mode == 2), labels
        assert net.status() & PF_STATUS_RANGE == PF_STATUS_RANGE, (mode, net.status())
        net.close()


def test_captured_forward_replays_equal_eager(force_conv, packs_down):
    """one captured forward with the down launch, replayed three times: the same bits as the eager forward every time"""
    from panoptic_forecasting_amd import lib as pflib
    L = pflib.load()
    force_conv(5, 2, 0, 0)
    g = torch.Generator().manual_seed(11)
    b, h, w = 2, 16, 40
    x = torch.randn(b, 12, h, w, generator=g).cuda()
    spec, P = down_net(g, 10, 28, 64)
    net = make_net(spec, P, 2)
    labels = run_labels(net, x)
    assert sum(DOWN in l for l in labels) == 1, labels
    want = {k: net.tensor(k).clone() for k in ('out', 'pl', 'nx')}

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
