"""conv_s4 folds of three-tile producers: the last 3x3 layer L4 of a HarDBlock with 33 .. 48 couts, on <3, 32, 8, 1>, also computes the
1x1 conv that reads its slice last.  down3 (plan option fold_down): the block's transition `dn` (ReLU, up to 96 couts) and its 2x2
average pool `pl`, as tests/test_gpu_fold_down.py for two tiles.  lo (plan option fold_lo): the block's output is upsampled (`up`) and
read by a 1x1 conv `cu` over [up, hi]; the schedule runs cu's columns over `up` at the low resolution into an fp32 scratch its other
half samples, and it is that launch the fold removes; L4's slice is stored only if something else reads it.

Option 2 against float64 torch and against the two launches (option 0) at the bars of tests/test_gpu_fold_final.py (assert_fold_close:
2e-5 (1 + max |ref|) and 1e-5 (1 + max |ref|)): the same products, another grouping of the fp32 sum.  A stored slice holds the same
bits in both modes.  Which kernels ran is read from the profile labels."""
import pytest
import torch
import torch.nn.functional as F

from test_fold_down_host import down_net
from test_fold_final_host import hard_block, random_params
from test_fold_wide_host import lo_net
from test_gpu_fold_down import DOWN, down_ref
from test_gpu_fold_final import TAIL, assert_fold_close, force_conv, raw_ranges, run_labels, slot_planes  # noqa: F401

pytestmark = pytest.mark.gpu

PF_STATUS_RANGE = 1
DOWN3 = 'conv_s4_down_kernel<3, 32, 8, 1>'
LO = 'conv_s4_lo_kernel<3, 32, 8, 1>'
PLAIN3 = 'conv_s4_kernel<3, 32, 8, 1>'


@pytest.fixture
def packs_wide():
    """plans are created with the fragments of every form packed whatever the process-wide values were, and mode 2 is what they start with"""
    from panoptic_forecasting_amd import lib as pflib
    L = pflib.load()
    for name in (b'fold_down', b'fold_lo', b'fold_final'):
        pflib.check(L.pf_set_option(name, 2), 'pf_set_option')
    yield
    for name in (b'fold_down', b'fold_lo', b'fold_final'):
        pflib.check(L.pf_set_option(name, 1), 'pf_set_option')


def block_ref(D, src, pre='', lead=0):
    """float64 hard_block over `src` -> (L2, out)"""
    cv = lambda n, t: F.relu(F.conv2d(t, *D[pre + n], padding=1))
    t0 = cv('t0', src)
    l1 = cv('L1', t0)
    l2 = cv('L2', torch.cat([l1, t0], 1))
    l3 = cv('L3', l2)
    l4 = cv('L4', torch.cat([l3, l2, t0], 1))
    return l2, torch.cat(([cv('L0', t0)] if lead else []) + [l1, l3, l4], 1)


def lo_ref(x, P, lead=0):
    D = {k: (v[0].double(), v[1].double()) for k, v in P.items()}
    hi = F.relu(F.conv2d(x.double(), *D['hi'], padding=1))
    s2 = F.relu(F.conv2d(x.double(), *D['s2'], padding=1, stride=2))
    l2, out = block_ref(D, s2, lead=lead)
    up = F.interpolate(out, size=hi.shape[-2:], mode='bilinear', align_corners=True)
    cu = F.relu(F.conv2d(torch.cat([up, hi], 1), *D['cu']))
    ref = {'L2': l2, 'out': out, 'cu': cu, 'nx': F.relu(F.conv2d(cu, *D['nx'], padding=1))}
    if 'sk' in D:
        ref['sk'] = F.conv2d(out, *D['sk'])
    return ref


def make_net(spec, P, mode, options=()):
    from helpers import MiniNet
    net = MiniNet(spec, P).set_option('fold_down', mode).set_option('fold_lo', mode).set_option('fuse_pairs', 0).set_option('share_s', 0)
    for name, value in options:
        net.set_option(name, value)
    return net


def check_wide(form, c_odd, c_even, r_cout, h, w, b, folded, options=(), modes=(0, 2), **kw):
    """h x w = L4's size (lo: the input is twice that).  Option 2 (or modes[1]) against float64 and against option 0; `folded`: the form's
    launch must have run (else the two launches).  With the slice elided (lo, no other reader) the block's output cannot be tapped and
    its L1 / L3 slices are compared as the bytes of their packed planes.  Returns the labels of the folded run"""
    g = torch.Generator().manual_seed(h * 7 + w + c_even + r_cout)
    hx, wx = (2 * h - (h & 1), 2 * w) if form == 'lo' else (h, w)          # (an odd h: a stride-2 conv of 2h - 1 rows)
    x = torch.randn(b, 12, hx, wx, generator=g) * torch.exp(0.5 * torch.randn(b, 12, 1, 1, generator=g))
    if form == 'lo':
        spec, P = lo_net(g, c_odd, c_even, r_cout, **kw)
        ref = lo_ref(x, P, kw.get('lead', 0))
    else:
        spec, P = down_net(g, c_odd, c_even, r_cout, **kw)
        ref = down_ref(x, P, kw.get('lead', 0), kw.get('r_relu', True), kw.get('pool', True))
    kernel = LO if form == 'lo' else DOWN3
    elided = form == 'lo' and folded and not kw.get('second_reader')
    front_groups = (kw.get('lead', 0) + 2 * c_odd) // 4
    got, labels, planes = {}, {}, {}
    for mode in modes:
        net = make_net(spec, P, mode, options)
        labels[mode] = run_labels(net, x)
        ran = any(kernel in l for l in labels[mode])
        assert ran == (folded and mode != 0), labels[mode]
        assert net.status() == 0
        got[mode] = {k: net.tensor(k).cpu() for k in ref if not (ran and elided and k == 'out')}
        if ran and elided:
            with pytest.raises(RuntimeError, match='elided'):       # the tap check
                net.tensor('out')
        planes[mode] = slot_planes(net, 'out', front_groups)
        net.close()
    two, fold = modes
    if folded:
        assert sum(kernel in l for l in labels[fold]) == 1, labels[fold]
        assert sum(PLAIN3 in l for l in labels[two]) == sum(PLAIN3 in l for l in labels[fold]) + 1, (labels[two], labels[fold])
        assert sum('conv_s4_1x1_kernel' in l for l in labels[two]) == sum('conv_s4_1x1_kernel' in l for l in labels[fold]) + 1
        assert len(labels[two]) == len(labels[fold]) + 1
        if form == 'down':
            assert not any('+pool' in l for l in labels[fold]), labels[fold]
    else:
        assert labels[two] == labels[fold]
    assert planes[two][0].any() and torch.equal(planes[two][0], planes[fold][0])      # the L1 / L3 slices: the same bits
    if elided:
        assert planes[two][1].any() and not planes[fold][1].any()                    # L4's slice: never stored by the lo launch
    else:
        assert planes[two][1].any() and torch.equal(planes[two][1], planes[fold][1])  # ... stored: the same bits
    assert_fold_close(ref, got[two], got[fold])
    return labels[fold]


# (form, c_odd, c_even, reader couts) at h x w (L4's size), batch b.  (16, 46, 63) lo and (16, 46, 96) down = FC-HarDNet-70's two pairs
# at 128 x 256: 32 channels in front of the slice; 8 x 32: one tile.  (4, 40, 17) lo: eight channels in front, eight couts in the
# third tile - chunks 0 and 2 mostly zeros -, one row in the reader's second tile.  (16, 48, 96) down at 16 x 64, two frames: full
# tiles everywhere, four workgroups a frame.  9 x 36 and 10 x 36: partial tiles in both directions, a last tile of four columns, an odd
# height (the pool drops the last row); the pooled width 18 is no multiple of 4: the pooled tensor is fp32
@pytest.mark.parametrize('form,c_odd,c_even,r_cout,h,w,b', [('lo', 16, 46, 63, 8, 32, 1), ('down', 16, 46, 96, 8, 32, 1), ('lo', 4, 40, 17, 8, 32, 1),
                                                            ('down', 16, 48, 96, 16, 64, 2), ('down', 16, 46, 96, 9, 36, 1),
                                                            ('down', 16, 46, 96, 10, 36, 2), ('lo', 16, 46, 63, 9, 36, 1),
                                                            ('lo', 16, 46, 63, 10, 36, 2)])
def test_fold_vs_float64_and_two_launches(form, c_odd, c_even, r_cout, h, w, b, force_conv, packs_wide):
    force_conv(5, 3, 0, 0)
    check_wide(form, c_odd, c_even, r_cout, h, w, b, True)


def test_second_reader_of_the_block_output_reads_what_the_down_fold_stored(force_conv, packs_wide):
    """`sk`, a 1x1 conv over the block's output behind the pool (the decoder's skip connection), with the fold on"""
    force_conv(5, 3, 0, 0)
    check_wide('down', 16, 46, 96, 16, 40, 2, True, skip=True)


def test_second_reader_of_the_block_output_makes_the_lo_fold_store_the_slice(force_conv, packs_wide):
    """`sk` reads the block's output too: the lo launch stores L4's slice as the plain launch does, the tensor can be tapped, sk is right"""
    force_conv(5, 3, 0, 0)
    check_wide('lo', 16, 46, 63, 16, 40, 2, True, second_reader=True)


def all_forms_net(g):
    """every form in one table: block A (10, 28) + `dn` (64) + `pl` [down]; block B (16, 46) over pl + `dn2` (96) + `pl2` [down3];
    block C (16, 46) over pl2, `up` to pl's size, `cu` (63) over [up, pl] [lo]; block D (10, 28) over cu + `fin` (11, no ReLU) [tail]"""
    from helpers import MiniSpec
    from panoptic_forecasting_amd import hardnet_arch as arch
    S = arch.Src
    spec, shapes = MiniSpec(12), []
    a, a_ch = hard_block(spec, shapes, S(0, 0, 12), 10, 28, pre='a.')
    pl = spec.pool('pl', spec.conv('dn', [S(a, 0, a_ch)], 64, 1))
    b, b_ch = hard_block(spec, shapes, S(pl, 0, 64), 16, 46, pre='b.')
    pl2 = spec.pool('pl2', spec.conv('dn2', [S(b, 0, b_ch)], 96, 1))
    c, c_ch = hard_block(spec, shapes, S(pl2, 0, 96), 16, 46, pre='c.')
    up = spec.upsample('up', c, pl)
    cu = spec.conv('cu', [S(up, 0, c_ch), S(pl, 0, 64)], 63, 1)
    d, d_ch = hard_block(spec, shapes, S(cu, 0, 63), 10, 28, pre='d.')
    spec.conv('fin', [S(d, 0, d_ch)], 11, 1, relu=False)
    shapes += [('dn', a_ch, 64, 1), ('dn2', b_ch, 96, 1), ('cu', c_ch + 64, 63, 1), ('fin', d_ch, 11, 1)]
    return spec, random_params(g, shapes)


def test_all_forms_in_one_plan(force_conv, packs_wide):
    """tail, down of two and of three tiles and lo: the schedule's fold pass runs once per form over the same step list.  One launch of
    each, none of the four 1x1 convs folded on its own; against float64 and against the same net with the options 0.  (conv_s4 with two
    cout tiles per workgroup: the three-tile layers are asked for three by the table of the rule's sizes only, so here they are forced)"""
    from helpers import MiniNet
    force_conv(5, 3, 0, 0)
    g = torch.Generator().manual_seed(21)
    x = torch.randn(1, 12, 16, 64, generator=g) * torch.exp(0.5 * torch.randn(1, 12, 1, 1, generator=g))
    spec, P = all_forms_net(g)
    D = {k: (v[0].double(), v[1].double()) for k, v in P.items()}
    ref = {}
    ref['a.L2'], ref['a.out'] = block_ref(D, x.double(), 'a.')
    ref['pl'] = F.avg_pool2d(F.relu(F.conv2d(ref['a.out'], *D['dn'])), 2)
    ref['b.L2'], ref['b.out'] = block_ref(D, ref['pl'], 'b.')
    ref['pl2'] = F.avg_pool2d(F.relu(F.conv2d(ref['b.out'], *D['dn2'])), 2)
    ref['c.L2'], c_out = block_ref(D, ref['pl2'], 'c.')
    up = F.interpolate(c_out, size=ref['pl'].shape[-2:], mode='bilinear', align_corners=True)
    ref['cu'] = F.relu(F.conv2d(torch.cat([up, ref['pl']], 1), *D['cu']))
    ref['d.L2'], d_out = block_ref(D, ref['cu'], 'd.')
    ref['fin'] = F.conv2d(d_out, *D['fin'])
    got, labels = {}, {}
    for mode in (0, 2):
        net = MiniNet(spec, P).set_option('fuse_pairs', 0).set_option('share_s', 0)
        for name in ('fold_final', 'fold_down', 'fold_lo'):
            net.set_option(name, mode)
        labels[mode] = run_labels(net, x)
        assert net.status() == 0
        got[mode] = {k: net.tensor(k).cpu() for k in ref}
        if mode == 2:
            for k in ('c.out', 'd.out'):                             # their last slices are elided
                with pytest.raises(RuntimeError, match='elided'):
                    net.tensor(k)
        net.close()
    # A's and D's last layers have two cout tiles: a request for three resolves to <2, 32, 8, 1>
    for kernel in (TAIL, DOWN, DOWN3, LO):
        assert sum(kernel in l for l in labels[2]) == 1, (kernel, labels[2])
    assert not any('tail' in l or 'down' in l or '_lo_' in l for l in labels[0]), labels[0]
    assert sum('conv_s4_1x1_kernel' in l for l in labels[0]) == sum('conv_s4_1x1_kernel' in l for l in labels[2]) + 4
    assert len(labels[0]) == len(labels[2]) + 4
    assert_fold_close(ref, got[0], got[2])


@pytest.mark.parametrize('form', ['down', 'lo'])
def test_k_split_shape_falls_back(form, force_conv, packs_wide):
    """8 x 32 tiles with two wave groups splitting L4's rounds: the forms are built without a K split"""
    force_conv(5, 3, 3, 0)
    labels = check_wide(form, 16, 46, 63, 16, 40, 2, False)
    assert any(', 32, 8, 2>' in l and 'conv_s4_kernel' in l for l in labels), labels


@pytest.mark.parametrize('form', ['down', 'lo'])
def test_add_launch_of_a_share_pair_falls_back(form, force_conv, packs_wide):
    """share_s = 2: L4 runs as the add launch of the pair (L3, L4)"""
    force_conv(5, 3, 0, 0)
    labels = check_wide(form, 16, 46, 63, 16, 40, 2, False, options=(('share_s', 2),))
    assert any('conv_s4_add_kernel' in l for l in labels), labels


@pytest.mark.parametrize('form', ['down', 'lo'])
def test_two_tiles_per_workgroup_fall_back(form, force_conv, packs_wide):
    """L4's three cout tiles in two workgroups of <2, 32, 8, 1>: no workgroup holds the whole slice"""
    force_conv(5, 2, 0, 0)
    labels = check_wide(form, 16, 46, 63, 16, 40, 2, False)
    assert any('conv_s4_kernel<2, 32, 8, 1>' in l for l in labels), labels


@pytest.mark.parametrize('form', ['down', 'lo'])
def test_rule_leaves_small_launches_alone(form, force_conv, packs_wide):
    """options at 1: launches of a class nobody measured stay two launches"""
    force_conv(5, 3, 0, 0)
    labels = check_wide(form, 16, 46, 63, 16, 40, 1, False, modes=(0, 1))
    assert any(PLAIN3 in l for l in labels), labels


@pytest.mark.parametrize('form,layer,scale', [('down', 'L4', 17), ('down', 'dn', 17), ('lo', 'L4', 17), ('down', 'L4', -24), ('lo', 'L4', -24)])
def test_range_guard_raises_the_same_bits_as_the_two_launches(form, layer, scale, force_conv, raw_ranges, packs_wide):
    """L4's weights and bias times 2^17: its slice (stored or elided) exceeds 65504.  dn's: the slice is in range, the pooled values are
    not.  Times 2^-24: the slice's maximum lies below the low bar.  The status word with the fold on is the one with it off"""
    force_conv(5, 3, 0, 0)
    g = torch.Generator().manual_seed(9)
    lo = form == 'lo'
    x = torch.randn(1, 12, 32 if lo else 16, 80 if lo else 40, generator=g)
    spec, P = lo_net(g, 16, 46, 63) if lo else down_net(g, 16, 46, 96)
    P[layer] = (P[layer][0] * 2.0 ** scale, P[layer][1] * 2.0 ** scale)
    ref = lo_ref(x, P) if lo else down_ref(x, P)
    if scale < 0:
        assert 0 < ref['out'][:, 32:].max().item() < 2.0 ** -10
    elif layer == 'L4':
        assert ref['out'].max().item() > 65504.0
    else:
        assert ref['out'].max().item() < 65504.0 / 64 and ref['pl'].max().item() > 65504.0
    status = {}
    for mode in (0, 2):
        net = make_net(spec, P, mode)
        labels = run_labels(net, x)
        assert any((LO if lo else DOWN3) in l for l in labels) == (mode == 2), labels
        status[mode] = net.status()
        net.close()
    assert status[0] == status[2], status
    if scale > 0:
        assert status[2] & PF_STATUS_RANGE == PF_STATUS_RANGE, status


@pytest.mark.parametrize('form', ['down', 'lo'])
def test_captured_forward_replays_equal_eager(form, force_conv, packs_wide):
    """one captured forward with the folded launch, replayed five times: the same bits as the eager forward every time"""
    from panoptic_forecasting_amd import lib as pflib
    L = pflib.load()
    force_conv(5, 3, 0, 0)
    g = torch.Generator().manual_seed(11)
    lo = form == 'lo'
    b, h, w = (2, 32, 80) if lo else (2, 16, 40)
    x = torch.randn(b, 12, h, w, generator=g).cuda()
    spec, P = lo_net(g, 16, 46, 63) if lo else down_net(g, 16, 46, 96)
    net = make_net(spec, P, 2)
    labels = run_labels(net, x)
    assert sum((LO if lo else DOWN3) in l for l in labels) == 1, labels
    want = {k: net.tensor(k).clone() for k in (('L2', 'cu', 'nx') if lo else ('out', 'pl', 'nx'))}

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
        for k in want:
            assert torch.equal(net.tensor(k), want[k]), (rep, k)
        assert net.status() == 0
    net.close()
