"""The fg forward (csrc/fg_net.hip enqueues what csrc/fg_schedule.cpp decides; kernels: fg_gemm.hip, fg_traj.hip) stage by stage against float64, through FGModel.forward alone.

Two devices make a stage observable from outside: the kernels' own public outputs (mask_feats, output_feats) are the reference's
INPUT for the stage behind them, and crafted weights (fg_ref64.crafted) turn the layers around a stage into exact identities - on the
matrix path an identity layer is one product by 1.0 plus zeros, so it hands its input on bit for bit (a ReLU aside).

Single-kernel cases, bar D (derived, elementwise, the form of stem_ref64.stem_bar):
    |hip - ref64| <= 1.01 (2K + 2) 2^-24 (op(|x|, |w|) + |b|)
with op the same linear operation in float64 on absolute values, x the kernel's own fp32 input and K the reduction length: the bound
of an fp32 sum of K rounded products and a bias in any order.  ReLU is 1-Lipschitz, so the bar holds behind it.  The cell case adds
the measured slack of the transcendental functions (see the test).

Stages that cannot be isolated, bar P (the project's measured bar, DESIGN section 4, the G8 row): per tensor
    max|hip - ref64| <= 2 max|ref32 - ref64| + 1e-6 (1 + max|ref64|)
ref32 / ref64 = the same checker function on the GPU in float32 / float64 with TF32 off.

Every case prints its worst err / bar and writes it to fg_probe_dist.json in the suite's scratch report directory
(tests/helpers.py: fg_probe_record); the MI355X run is kept as profiles/fg_probe_dist.json.
"""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import fg_ref64 as R
from helpers import fg_probe_record

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
OUTS = ('normalized_trajectory', 'unnormalized_trajectory', 'mask_feats', 'output_feats', 'masks')
U = 2.0 ** -24
HOT_GAIN = 16.0           # tests/test_fg_host.py::test_hot_weights_saturate_the_first_cell: the same gain meets the condition at N = 1


@pytest.fixture(scope='module')
def model():
    from panoptic_forecasting_amd.registry import build_model
    p = R.fg_params()
    p['no_gpu'] = False
    m = build_model(p)
    m.load_state_dict(R.fill_weights(m.state_dict()))
    return m


@pytest.fixture(scope='module')
def base(model):
    """the base fill on the device, fp32: never modified"""
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


@pytest.fixture(scope='module')
def base64(base):
    return {k: v.double() for k, v in base.items()}


@pytest.fixture(scope='module', autouse=True)
def tf32_off():
    was = torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = torch.backends.cudnn.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = was


@contextlib.contextmanager
def loaded(model, base, items):
    """the crafted set ``items`` in the model (only the replaced tensors are copied; their version counters make the next forward
    pack again), the base fill back on the way out -> the crafted state_dict"""
    sd = R.crafted(base, items)
    new = {k: v for k, v in sd.items() if v is not base[k]}
    model.load_state_dict(new, strict=False)
    try:
        yield sd
    finally:
        model.load_state_dict({k: base[k] for k in new}, strict=False)


def _args(case, n, t_in, t_out, classes=None, **kw):
    inputs, labels = R.make_inputs(case, [n], t_in=t_in, t_out=t_out, **kw)
    a = [x.to(DEV) if torch.is_tensor(x) else x for x in R.forward_args(inputs, labels)]
    if classes is not None:
        a[8] = torch.as_tensor(classes, dtype=torch.long, device=DEV)
    return a


def _ratio(got, ref, bar):
    """worst |got - ref| / bar; a zero bar passes only an exact value"""
    err = (got.double() - ref).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bar.clamp_min(1e-300)).max())


def _copies(masks):
    """[N, 28, 28] -> [N, 14, 14, 4]: the four (dy, dx) positions of every source pixel"""
    n = masks.size(0)
    return masks.reshape(n, 14, 2, 14, 2).permute(0, 1, 3, 2, 4).reshape(n, 14, 14, 4)


def _ident(ks):
    return [('ident_fcn', k) for k in ks]


CLASSES16 = [k % 8 for k in range(16)]              # every class twice


# --------------------------------------------------------------------------------------------- 2. one kernel at a time, bar D
@pytest.mark.parametrize('pos,chans', [(1, R.ONEHOT_A), (4, R.ONEHOT_B)], ids=['fcn1-A', 'fcn4-B'])
def test_fcn_3x3_relu_alone(model, base, pos, chans):
    """gemm_kernel<9, relu>: mask_fcn<pos> from the base fill, the other three identities, the deconvolution a replication, the
    predictor a selection of channel chans[class].  pos = 4: the input is relu(output_feats) and the layer writes the other
    ping-pong buffer."""
    n, K = 16, 256 * 9
    args = _args(30 + pos, n, 1, 1, classes=CLASSES16)
    with loaded(model, base, _ident([k for k in (1, 2, 3, 4) if k != pos]) + ['replicate_deconv', ('onehot_predictor', chans)]) as sd:
        out = model(*args)
        cp = _copies(out['masks'])
    for j in (1, 2, 3):
        assert torch.equal(cp[..., j], cp[..., 0]), 'the four (dy, dx) copies differ'
    x = out['output_feats'].double()
    if pos != 1:
        x = F.relu(x)
    w, b = sd['mask_head.mask_fcn%d.weight' % pos].double(), sd['mask_head.mask_fcn%d.bias' % pos].double()
    ch = torch.tensor(chans, device=DEV)[args[8]]
    rows = torch.arange(n, device=DEV)
    ref = F.relu(F.conv2d(x, w, b, padding=1))[rows, ch]
    bar = 1.01 * (2 * K + 2) * U * F.conv2d(x.abs(), w.abs(), b.abs(), padding=1)[rows, ch]
    r = _ratio(cp[..., 0], ref, bar)
    print('mask_fcn%d: worst err / bar D = %.4g (K = %d, max|ref| %.3g)' % (pos, r, K, float(ref.abs().max())))
    fg_probe_record('2.1 fcn%d' % pos, {'err_over_bar': float('%.4g' % r), 'K': K, 'kernel': 'gemm_kernel<9,relu>'})
    assert float(ref.abs().max()) > 0.1 and r <= 1.0


@pytest.mark.parametrize('chans', [R.ONEHOT_A, R.ONEHOT_B], ids=['A', 'B'])
def test_deconv_pixel_shuffle_alone(model, base, chans):
    """gemm_kernel<1, deconv>: all 784 pixels of channel chans[class]: the q -> (co, dy, dx) split and bias[co]"""
    n, K = 16, 256
    args = _args(35, n, 1, 1, classes=CLASSES16)
    with loaded(model, base, _ident((1, 2, 3, 4)) + [('onehot_predictor', chans)]) as sd:
        out = model(*args)
    y = F.relu(out['output_feats'].double())
    w, b = sd['mask_head.deconv.weight'].double(), sd['mask_head.deconv.bias'].double()
    ch = torch.tensor(chans, device=DEV)[args[8]]
    rows = torch.arange(n, device=DEV)
    ref = F.relu(F.conv_transpose2d(y, w, b, stride=2))[rows, ch]
    bar = 1.01 * (2 * K + 2) * U * F.conv_transpose2d(y, w.abs(), b.abs(), stride=2)[rows, ch]
    r = _ratio(out['masks'], ref, bar)
    print('deconv: worst err / bar D = %.4g (K = %d, max|ref| %.3g)' % (r, K, float(ref.abs().max())))
    fg_probe_record('2.2 deconv %s' % ('A' if chans == R.ONEHOT_A else 'B'),
                    {'err_over_bar': float('%.4g' % r), 'K': K, 'kernel': 'gemm_kernel<1,deconv>'})
    assert float(ref.abs().max()) > 0.1 and r <= 1.0


def test_predictor_alone(model, base):
    """predictor_kernel: the class row of a random predictor over replicated relu(output_feats)"""
    n, K = 16, 256
    args = _args(36, n, 1, 1, classes=CLASSES16)
    with loaded(model, base, _ident((1, 2, 3, 4)) + ['replicate_deconv']) as sd:
        out = model(*args)
    y = F.relu(out['output_feats'].double()).repeat_interleave(2, -2).repeat_interleave(2, -1)
    w = sd['mask_head.predictor.weight'].double()[args[8], :, 0, 0]
    b = sd['mask_head.predictor.bias'].double()[args[8]][:, None, None]
    ref = torch.einsum('nchw,nc->nhw', y, w) + b
    bar = 1.01 * (2 * K + 2) * U * (torch.einsum('nchw,nc->nhw', y, w.abs()) + b.abs())
    r = _ratio(out['masks'], ref, bar)
    print('predictor: worst err / bar D = %.4g (K = %d, max|ref| %.3g)' % (r, K, float(ref.abs().max())))
    fg_probe_record('2.3 predictor', {'err_over_bar': float('%.4g' % r), 'K': K, 'kernel': 'predictor_kernel'})
    assert float(ref.abs().max()) > 1.0 and r <= 1.0


def test_gather_every_index_in_one_batch(model):
    n, t_out = 16, 3
    inds = [k % t_out for k in range(n)]
    args = _args(37, n, 1, t_out, output_inds=inds)
    out = model(*args)
    mf = out['mask_feats']
    rows = torch.arange(n, device=DEV)
    assert torch.equal(out['output_feats'], mf[rows, 1 + args[4]])
    assert torch.equal(out['output_feats'], R.gather64(mf, args[4]))
    for s in range(t_out + 1):                       # no two slots alike: a wrong slot cannot pass
        for s2 in range(s):
            assert not torch.equal(mf[:, s], mf[:, s2])


def test_first_cell_alone(model, base):
    """gemm_kernel<9, lstm> with h == nullptr and the vec source, at one input step.  ident_out_conv makes mask_feats[:, 0] layer 1's
    h exactly; transparent_cell1 makes that h = tanh(tanh(h0)) in fp32 (sigmoid(20) = 1), a 1-Lipschitz image of cell 0's output
    h0 = s(o) tanh(s(i) tanh(g)) (c_prev = 0: f does not enter); const_traj_feat makes the 16 plane-constant channels exactly the
    bias (+-1.5 ... 2.2, the weight of the feature planes), so x below IS the kernel's fp32 input.  Reference: forward64 on the same
    weights.  Bar: the derived bound of the three pre-activations, K = 272 * 9, through |dh0/di| <= 1/4, |dh0/dg| <= 1,
    |dh0/do| <= 1/4, plus s = 2 s0, s0 = the measured distance of torch's own fp32 sigmoid / tanh chain from float64 on the
    float64 pre-activations rounded to fp32 (it stands for __expf / tanhf)."""
    n, K = 16, 272 * 9
    args = _args(38, n, 1, 1)
    cell = 'mask_encoder.cell_list.0.conv'
    with loaded(model, base, ['ident_out_conv', 'transparent_cell1', ('const_traj_feat', 1.5)]) as sd:
        out = model(*args)
        got = out['mask_feats'][:, 0].clone()
    with torch.no_grad():
        ref = R.forward64(sd, *args)['mask_feats'][:, 0]
        x = torch.cat([sd['traj_feat_out.bias'].double()[None, :, None, None].expand(n, -1, 14, 14), args[3][:, 0].double()], 1)
        w, b = sd[cell + '.weight'].double()[:, :272], sd[cell + '.bias'].double()
        z = torch.zeros(n, 256, 14, 14, dtype=torch.float64, device=DEV)
        i, _, o, g = R.cell64(sd, cell, x, z, z, gates=True)[2]
        A = F.conv2d(x.abs(), w.abs(), b.abs(), padding=1)                     # K half of h: zero state, weights never read
        Ai, _, Ao, Ag = A.chunk(4, 1)
        chain = lambda i, o, g: torch.tanh(torch.tanh(torch.sigmoid(o) * torch.tanh(torch.sigmoid(i) * torch.tanh(g))))
        s0 = float((chain(i.float(), o.float(), g.float()).double() - chain(i, o, g)).abs().max())
    bar = 1.01 * (2 * K + 2) * U * (0.25 * Ai + Ag + 0.25 * Ao) + 2 * s0
    edge = torch.zeros(14, 14, dtype=torch.bool, device=DEV)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    q = (got.double() - ref).abs() / bar
    r, r_edge, r_in = float(q.max()), float(q[..., edge].max()), float(q[..., ~edge].max())
    print('first cell: worst err / bar = %.4g (border pixels %.4g, interior %.4g); s0 = %.3g, max err %.3g, pre-activation std %.3g'
          % (r, r_edge, r_in, s0, float((got.double() - ref).abs().max()), float(torch.cat([i, o, g]).std())))
    fg_probe_record('2.5 first cell', {'err_over_bar': float('%.4g' % r), 'border': float('%.4g' % r_edge), 'interior': float('%.4g' % r_in),
                                       's0': float('%.4g' % s0), 'K': K, 'kernel': 'gemm_kernel<9,lstm>, h = nullptr'})
    assert float(ref.abs().max()) > 0.3 and r <= 1.0


# ------------------------------------------------------------------------------------- 3. decoupled references, bar P
def _bar_p(got, r64, r32):
    """(max err, bar, the fp32 checker's own distance) of one tensor"""
    e32 = float((r32.double() - r64).abs().max())
    return float((got.double() - r64).abs().max()), 2 * e32 + 1e-6 * (1 + float(r64.abs().max())), e32


def _check_p(case_id, got, r64, r32, slots=()):
    """bar P per tensor of ``got``; ``slots``: tensors whose err / bar is also reported per index of dimension 1"""
    entry, bad = {}, []
    for k in got:
        err, bar, e32 = _bar_p(got[k], r64[k], r32[k])
        entry[k] = {'err': float('%.4g' % err), 'bar': float('%.4g' % bar), 'e32': float('%.4g' % e32), 'err_over_bar': float('%.4g' % (err / bar))}
        if k in slots:
            entry[k]['err_per_slot'] = [float('%.3g' % float((got[k][:, s].double() - r64[k][:, s]).abs().max())) for s in range(got[k].size(1))]
        assert bool(torch.isfinite(got[k]).all()), k
        if not err <= bar:
            bad.append((k, err, bar))
    worst = max(v['err_over_bar'] for v in entry.values())
    print('%s: worst err / bar P = %.4g  %s' % (case_id, worst, {k: (v['err'], v['bar']) for k, v in entry.items()}))
    fg_probe_record(case_id, entry)
    return bad


MATRIX = [(t_in, t_out, 0, 'fixture') for t_in, t_out in ((1, 1), (1, 3), (2, 1), (2, 16), (4, 2), (16, 1), (16, 16))] + \
         [(1, 3, 2, 'fixture'), (4, 2, 2, 'fixture')] + \
         [(t_in, t_out, 0, mode) for t_in, t_out in ((4, 2), (16, 1)) for mode in ('absent', 'alternate', 'wide')]


@pytest.mark.parametrize('t_in,t_out,surplus,mode', MATRIX, ids=['%d-%d%s-%s' % (a, b, '+%d' % c if c else '', d) for a, b, c, d in MATRIX])
def test_step_counts_odometry_rows_and_masks(model, base, base64, t_in, t_out, surplus, mode):
    """The whole forward at N = 3 over the step-count matrix (the layer-0 ring of max(T_in, 2) slots and its wrap in the decoder,
    the layer-1 ping-pong phase, the h == nullptr first step), with surplus odometry rows filled with 1e3 (a wrong row stride or
    decoder row cannot pass) and the mask modes of fg_ref64.make_inputs.  All five outputs against forward64 from the inputs, and the
    trajectory path against traj64 fed the kernels' own mask_feats (the ConvLSTM's error is then not in the reference)."""
    n = 3
    inputs, labels = R.make_inputs(40 + t_in + t_out, [n], t_in=t_in, t_out=t_out, odom_t=t_in + t_out + surplus, mask_mode=mode)
    a = [x.to(DEV) if torch.is_tensor(x) else x for x in R.forward_args(inputs, labels)]
    if surplus:
        a[5][:, t_in + t_out:] = 1e3
    call = list(a)
    if mode == 'wide':                               # forward itself gets the wide masks; the checker the sliced ones
        call[1] = torch.cat(inputs['bbox_masks']).float().to(DEV)
        call[2] = torch.cat(inputs['bbox_vel_masks']).float().to(DEV)
        assert call[1].shape == (n, t_in + R.WIDE_EXTRA) and a[1].shape == (n, t_in)
    out = model(*call)
    assert out['mask_feats'].shape == (n, 1 + t_out, 256, 14, 14) and out['normalized_trajectory'].shape == (n, 1 + t_out, 10)
    name = '%d/%d%s %s' % (t_in, t_out, ' +%d odometry rows' % surplus if surplus else '', mode)
    with torch.no_grad():
        r64 = R.forward64(base64, *a)
        r32 = R.forward64(base, *a, dtype=torch.float32)
        bad = _check_p('3.2 ' + name, {k: out[k] for k in OUTS}, r64, r32, slots=('mask_feats', 'normalized_trajectory'))
        ta = (a[0], a[1], a[2], a[3], a[5], a[6], a[7], t_out, out['mask_feats'])
        t64 = R.traj64(base64, *ta)
        t32 = R.traj64(base, *ta, dtype=torch.float32)
        keys = ('normalized_trajectory', 'unnormalized_trajectory')
        bad += _check_p('3.1 ' + name, {k: out[k] for k in keys}, t64, t32, slots=keys)
    assert not bad, bad
    if mode == 'absent':
        # instance n - 1 is masked at every step: its input features reach the encoder only times 0
        feats2 = a[3].clone()
        feats2[n - 1] *= 2
        call[3] = feats2
        out2 = model(*call)
        assert torch.equal(out2['normalized_trajectory'][n - 1, 0], out['normalized_trajectory'][n - 1, 0])
        assert not torch.equal(out2['mask_feats'][n - 1], out['mask_feats'][n - 1])              # ... while the ConvLSTM does see them
        assert torch.equal(out2['mask_feats'][:n - 1], out['mask_feats'][:n - 1])


def test_saturated_gates(model, base):
    """ConvLSTM weights times HOT_GAIN at 3 / 3, N = 4: sigm = 1 / (1 + __expf(-x)) and tanhf in their tails, a cell state that grows
    over the steps.  The condition is asserted on the float64 reference alone: >= 5 % of cell 0's first pre-activations beyond +-10, the
    largest beyond +-20.

    This is the test that made gemm_kernel<9, .> sum each 72-deep round into partials of its own: with all of K (up to 1188 matrix
    steps) on one accumulator, mask_feats were 6.329e-4 from float64 against a bar of 6.279e-4 (err / bar 1.008) and output_feats
    1.106, the fp32 checker itself being 3.1e-4 away (at this gain a rounding error grows about 10^3-fold over the twelve cell
    evaluations, for both).  With the blocked sum: 1.57e-4 and 1.27e-4, worst err / bar 0.25 ("fg summation order")."""
    args = _args(39, 4, 3, 3)
    taps = {}
    with loaded(model, base, ('hot', HOT_GAIN)) as sd:
        out = model(*args)
        out = {k: out[k].clone() for k in OUTS}
    with torch.no_grad():
        r64 = R.forward64(sd, *args, taps=taps)
        r32 = R.forward64(sd, *args, dtype=torch.float32)
    share, top = R.saturation(taps['cell0_pre'][0])
    late = R.saturation(taps['cell0_pre'][-1])
    print('gain %g: first cell %.1f %% beyond +-10, max %.1f; last decoder cell %.1f %%, max %.1f' % (HOT_GAIN, 100 * share, top, 100 * late[0], late[1]))
    assert share >= 0.05 and top > 20.0
    bad = _check_p('3.3 hot gain %g' % HOT_GAIN, out, r64, r32, slots=('mask_feats',))
    assert not bad, bad


def test_indices_and_classes_are_clamped(model):
    """gather_kernel clamps output_inds into [0, T_out), predictor_kernel classes into [0, 8), in 64 bits: a negative index goes to
    0 (torch indexing would wrap), 2^33 + 1 and 2^32 + 2 go to the top (their low 32 bits, 1 and 2, would be in range)"""
    t_out = 3
    args = _args(41, 3, 2, t_out)
    wild, tame = list(args), list(args)
    wild[4] = torch.tensor([-1, t_out, 2 ** 33 + 1], device=DEV)
    wild[8] = torch.tensor([-3, 8, 2 ** 32 + 2], device=DEV)
    tame[4] = torch.tensor([0, t_out - 1, t_out - 1], device=DEV)
    tame[8] = torch.tensor([0, 7, 7], device=DEV)
    a, b = model(*wild), model(*tame)
    for k in OUTS:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(b['output_feats'][0], b['mask_feats'][0, 1]) and torch.equal(b['output_feats'][2], b['mask_feats'][2, t_out])


def test_wrapper_conversions_keep_the_bits(model):
    """float64 trajectories / odometry / depths, bool masks and a non-contiguous feature view give the contiguous fp32 call's bits"""
    args = _args(42, 3, 2, 2)
    want = model(*args)
    other = list(args)
    for j in (0, 5, 6):
        other[j] = args[j].double()
    for j in (1, 2, 7):
        other[j] = args[j].bool()
    other[3] = args[3].permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    assert not other[3].is_contiguous() and torch.equal(other[3], args[3]) and other[7].shape == (3, 2, 1)
    got = model(*other)
    for k in OUTS:
        assert torch.equal(got[k], want[k]), k
