"""Test helper for the fg forecaster (not a test module): deterministic fills and a float64 functional checker.

Fills are counter-based, so the generator (tests/golden/make_golden_fgnet.py) and the tests rebuild the same weights and
inputs bit for bit without storing them:  u(s, i) = mix32(i * 0x9E3779B1 + (s + 1) * 0x85EBCA77) / 2^32  in [0, 1), where
mix32 is the murmur3 finaliser (x ^= x>>16; x *= 0x85EBCA6B; x ^= x>>13; x *= 0xC2B2AE35; x ^= x>>16, all mod 2^32),
``s`` the stream (the index of the state_dict key, or 1000 + 100*case + input number) and ``i`` the flat element index.

``forward64`` restates FGModel.forward in functional torch ops (conv2d / conv_transpose2d / matmul) for the supported
configuration (the shipped fg config); tests/test_fg_host.py pins it to the reference's own float64 run in the fixture.
It is composed of stage functions (``inst_feat64``, ``traj64``'s steps, ``cell64``, ``gather64``, ``head64``) that the stage tests
also call one at a time, and ``crafted`` builds the weight sets that make the layers around a stage exact identities.
"""
import numpy as np
import torch
import torch.nn.functional as F

T_IN = 3
ODOM = 5
TRAJ = 10          # 8 box values + 2 depths
HID = 128
TRAJ_MEAN = [1024., 512., 200., 150., 0., 0., 0., 0.]
TRAJ_STD = [300., 150., 60., 50., 10., 10., 5., 5.]
DEPTH_MEAN, DEPTH_STD = [20., 0.], [10., 2.]
ODOM_MEAN, ODOM_STD = [0.1, -0.2, 0., 5., 0.01], [1., 1., 0.5, 3., 0.1]
PREDICTOR_GAIN = 40.0     # the mask logits then span several units (the reference's std=0.001 init makes them ~0)

FG_CONFIG = {'inp_emb_size': 32, 'instance_feat_channels': 8, 'instance_feat_hidden': 64, 'loss_type': 'smoothl1',
             'mask_crossent_coef': 0.0, 'mask_distill_coef': 1.0,
             'mask_head': {'maskrcnn_pretrain_path': None, 'no_finetune': True},
             'model_type': 'segbbox_independent_ed', 'num_convlstm_layers': 2, 'num_traj_out_layers': 2,
             'rnn_hidden': 128, 'rnn_type': 'gru', 'traj_coef': 0.1, 'traj_feat_channels': 16, 'use_depth_inp': True,
             'use_full_instance_traj_inp': True, 'use_odometry': True}


def fg_params(**model_overrides):
    model = dict(FG_CONFIG)
    model.update(model_overrides)
    return {'task': 'fg', 'no_gpu': True, 'load_model': None, 'load_best_model': False, 'model': model,
            'data': {'odom_size': ODOM,
                     'norm_params': [torch.tensor(TRAJ_MEAN), torch.tensor(TRAJ_STD)],
                     'depth_norm_params': [torch.tensor(DEPTH_MEAN), torch.tensor(DEPTH_STD)],
                     'odom_norm_params': [torch.tensor(ODOM_MEAN), torch.tensor(ODOM_STD)]}}


def uniform(stream, n):
    m = np.uint64(0xFFFFFFFF)
    x = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B1) + np.uint64((stream + 1) * 0x85EBCA77)) & m
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & m
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & m
    x ^= x >> np.uint64(16)
    return x.astype(np.float64) / 4294967296.0


def sym(stream, shape, a):
    """uniform in [-a, a), float32."""
    n = int(np.prod(shape)) if len(shape) else 1
    return torch.from_numpy(((2 * uniform(stream, n) - 1) * a).astype(np.float32).reshape(shape))


def fill_weights(state_dict):
    """The fixture's weights for a state_dict of the shipped shapes (keys in state_dict order = the streams)."""
    out = {}
    norms = {'traj_mean': TRAJ_MEAN, 'traj_std': TRAJ_STD, 'depth_mean': DEPTH_MEAN, 'depth_std': DEPTH_STD,
             'odom_mean': ODOM_MEAN, 'odom_std': ODOM_STD}
    for s, (k, v) in enumerate(state_dict.items()):
        if k in norms:
            out[k] = torch.tensor(norms[k], dtype=torch.float32).reshape(v.shape)
        elif v.dim() == 1:
            out[k] = sym(s, tuple(v.shape), 0.1)
        else:
            fan_in = int(np.prod(v.shape[1:])) if not k.endswith('deconv.weight') else v.shape[0]
            a = (3.0 / fan_in) ** 0.5
            if k.endswith('predictor.weight'):
                a *= PREDICTOR_GAIN
            out[k] = sym(s, tuple(v.shape), a)
    return out


MASK_MODES = ('fixture', 'absent', 'alternate', 'wide')
WIDE_EXTRA = 2            # surplus mask columns of mask_mode 'wide'


def make_inputs(case, counts, t_out=3, odom_t=None, output_inds=None, masked=True, t_in=T_IN, mask_mode='fixture'):
    """Per-image lists (the reference's predict_* inputs) for ``counts`` instances; stream 1000 + 100*case + j.

    ``mask_mode`` (on top of the fixture's holes, where ``t_in`` has room for them):
      'absent'     the last instance has ``bbox_masks`` zero at every step, hence ``bbox_vel_masks`` zero
      'alternate'  ``depth_masks[n, t] = (t + n) even``: dm[t] * dm[t-1] is 0 everywhere, except that instance 0 has depth at its last
                   two steps too (the one place where the product is 1, given t_in >= 2)
      'wide'       ``bbox_masks`` / ``bbox_vel_masks`` have WIDE_EXTRA more columns than steps, all set: this project's
                   FGModel.forward slices them, as the reference's predict_* do before they call forward (``forward_args``);
                   ``depth_masks`` keeps t_in columns (the reference concatenates it unsliced)
    """
    assert mask_mode in MASK_MODES and t_in >= 1
    n = int(sum(counts))
    odom_t = odom_t or t_in + t_out
    base = 1000 + 100 * case
    u = lambda j, shape: torch.from_numpy(uniform(base + j, int(np.prod(shape))).astype(np.float32).reshape(shape))
    mean = torch.tensor(TRAJ_MEAN)
    std = torch.tensor(TRAJ_STD)
    trajs = mean + std * (2 * u(0, (n, t_in, 8)) - 1)
    depths = torch.tensor(DEPTH_MEAN) + torch.tensor(DEPTH_STD) * (2 * u(1, (n, t_in, 2)) - 1)
    odom = torch.tensor(ODOM_MEAN) + torch.tensor(ODOM_STD) * (2 * u(2, (n, odom_t, ODOM)) - 1)
    feats = u(3, (n, t_in, 256, 14, 14))
    mask = torch.ones(n, t_in)
    dmask = torch.ones(n, t_in, 1, dtype=torch.bool)
    if masked and n > 1:
        mask[1, 0] = 0                      # instance 1 is missing at the first input step
        if t_in > 1:
            dmask[1, 1, 0] = False          # ... and has no depth at the second
    if masked and n > 3 and t_in > 2:
        mask[3, 2] = 0                      # instance 3 is missing at the most recent input step
    if mask_mode == 'absent' and n:
        mask[n - 1] = 0
    if mask_mode == 'alternate':
        dmask[:, :, 0] = (torch.arange(t_in)[None, :] + torch.arange(n)[:, None]) % 2 == 0
        if n and t_in > 1:
            dmask[0, t_in - 2:, 0] = True
    vel = torch.zeros(n, t_in)
    vel[:, 1:] = mask[:, 1:] * mask[:, :-1]
    if mask_mode == 'wide':
        mask = torch.cat([mask, torch.ones(n, WIDE_EXTRA)], 1)
        vel = torch.cat([vel, torch.ones(n, WIDE_EXTRA)], 1)
    classes = (u(4, (n,)) * 8).long().clamp(max=7)
    if output_inds is None:
        output_inds = (u(5, (n,)) * t_out).long().clamp(max=t_out - 1)
    output_inds = torch.as_tensor(output_inds, dtype=torch.long).expand(n).clone()
    split = lambda t: list(t.split(list(counts)))
    inputs = {'trajectories': split(trajs), 'bbox_masks': split(mask.bool()), 'bbox_vel_masks': split(vel.bool()),
              'feats': split(feats), 'odometry': split(odom), 'depths': split(depths), 'depth_masks': split(dmask),
              'classes': split(classes)}
    labels = {'trajectories': split(torch.zeros(n, t_out, 8)), 'output_inds': split(output_inds)}
    return inputs, labels


def forward_args(inputs, labels):
    """The positional arguments predict_* hands to forward (fg_model.py:524-529)."""
    cat = lambda k: torch.cat(inputs[k])
    trajs = cat('trajectories')
    t_out = labels['trajectories'][0].size(1)
    return (trajs, cat('bbox_masks').float()[:, :trajs.size(1)], cat('bbox_vel_masks').float()[:, :trajs.size(1)],
            cat('feats'), torch.cat(labels['output_inds']), cat('odometry'), cat('depths'), cat('depth_masks'),
            cat('classes'), t_out)


def background(seed, b, h=1024, w=2048):
    """Blocky label maps with stuff (< 11), things (11..18) and 255."""
    uu = uniform(5000 + seed, b * (h // 64) * (w // 64)).reshape(b, h // 64, w // 64)
    low = np.floor(uu * 19).astype(np.int64)
    low[uniform(6000 + seed, low.size).reshape(low.shape) < 0.05] = 255
    return torch.from_numpy(low.repeat(64, 1).repeat(64, 2))


def _base_map(background, panoptic):
    base = np.asarray(background).astype(np.int64).copy()
    if panoptic:
        base[base >= 11] = 255                  # fg_model.py:516-517
    return base


def seg_overlay(seg, background, panoptic):
    """uint16 map of the pixels where ``seg`` differs from the instance-free result, 0 elsewhere (instance values are >= 11)."""
    seg = np.asarray(seg).astype(np.int64)
    out = np.where(seg != _base_map(background, panoptic), seg, 0)
    assert out.min() >= 0 and out.max() < 65536
    return out.astype(np.uint16)


def seg_from_overlay(overlay, background, panoptic):
    """The full map back from ``seg_overlay``."""
    overlay = np.asarray(overlay).astype(np.int64)
    return np.where(overlay != 0, overlay, _base_map(background, panoptic))


# ---------------------------------------------------------------------------------------------- float64 checker
def _gru(x, h, w_ih, w_hh, b_ih, b_hh):
    gi = x @ w_ih.t() + b_ih
    gh = h @ w_hh.t() + b_hh
    ir, iz, inn = gi.chunk(3, -1)
    hr, hz, hn = gh.chunk(3, -1)
    r = torch.sigmoid(ir + hr)
    z = torch.sigmoid(iz + hz)
    nn_ = torch.tanh(inn + r * hn)
    return (1 - z) * nn_ + z * h


def _mlp(sd, pre, h):
    h = F.relu(h @ sd[pre + '.0.weight'].t() + sd[pre + '.0.bias'])
    return h @ sd[pre + '.2.weight'].t() + sd[pre + '.2.bias']


def _cast(sd, d):
    return {k: v.to(d) for k, v in sd.items()}


def _plane(v):
    return v[:, :, None, None].expand(-1, -1, 14, 14)


# ---- the stages.  forward64 below is composed of exactly these calls, so a stage fed with forward64's own intermediate tensors
#      returns forward64's bits (tests/test_fg_host.py), and fed with the kernels' public outputs it is the reference of the stage
#      behind them alone (tests/test_gpu_fg_stages.py).
def cell64(sd, pre, x, h, c, dtype=torch.float64, gates=False):
    """One ConvLSTM cell (convlstm.py:44-68), gate rows i, f, o, g -> (h', c'), with ``gates`` also the four pre-activations."""
    sd = _cast({k: sd[k] for k in (pre + '.weight', pre + '.bias')}, dtype)
    g = F.conv2d(torch.cat([x.to(dtype), h.to(dtype)], 1), sd[pre + '.weight'], sd[pre + '.bias'], padding=1)
    i, f, o, gg = g.chunk(4, 1)
    c = torch.sigmoid(f) * c.to(dtype) + torch.sigmoid(i) * torch.tanh(gg)
    h = torch.sigmoid(o) * torch.tanh(c)
    return (h, c, (i, f, o, gg)) if gates else (h, c)


def inst_feat64(sd, feats, dtype=torch.float64):
    """_compute_traj_inst_feats without the mask: feats [N, 256, 14, 14] -> [N, 64]."""
    w = lambda k: sd[k].to(dtype)
    x = F.conv2d(feats.to(dtype), w('instance_compressor.weight'), w('instance_compressor.bias'))
    x = F.relu(x.reshape(x.size(0), -1))
    return x @ w('instance_feat_model.weight').t() + w('instance_feat_model.bias')


def _traj_encode(sd, trajs, traj_mask, vel_mask, feats, odom, depths, depth_masks, d):
    """normalisation, expand_traj_mask and the encoder GRU -> (normalised odometry, [h_t], mean, std); sd already in ``d``"""
    dev = trajs.device
    trajs, feats, odom, depths = trajs.to(d), feats.to(d), odom.to(d), depths.to(d)
    m = traj_mask.to(d)
    vm = vel_mask.to(d)
    dm = depth_masks.to(d).reshape(m.shape)
    n, t_in = m.shape
    mean = torch.cat([sd['traj_mean'], sd['depth_mean']], -1)
    std = torch.cat([sd['traj_std'], sd['depth_std']], -1)
    dvel = torch.cat([torch.zeros(n, 1, dtype=d, device=dev), dm[:, 1:] * dm[:, :-1]], 1)
    emask = torch.cat([m[..., None].expand(-1, -1, 4), vm[..., None].expand(-1, -1, 4), dm[..., None], dvel[..., None]], -1)
    x = (torch.cat([trajs, depths], -1) - mean) / std * emask
    odom = (odom - sd['odom_mean']) / sd['odom_std']
    hdim = sd['traj_encoder.weight_hh_l0'].shape[1]
    h = torch.zeros(n, hdim, dtype=d, device=dev)
    enc_h = []
    for t in range(t_in):
        inst = inst_feat64(sd, feats[:, t], d) * m[:, t:t + 1]
        h = _gru(torch.cat([x[:, t], inst, m[:, t:t + 1], odom[:, t]], -1), h, sd['traj_encoder.weight_ih_l0'],
                 sd['traj_encoder.weight_hh_l0'], sd['traj_encoder.bias_ih_l0'], sd['traj_encoder.bias_hh_l0'])
        enc_h.append(h)
    return odom, enc_h, mean, std


def _traj_step(sd, cur, h, cmf, odom_row, d):
    """one decoder step (fg_model.py:289-309) on the current mask features ``cmf`` -> (current_traj, h)"""
    inst = inst_feat64(sd, cmf, d)
    h = _gru(torch.cat([cur, inst, odom_row], -1), h, sd['traj_decoder.weight_ih_l0'],
             sd['traj_decoder.weight_hh_l0'], sd['traj_decoder.bias_ih_l0'], sd['traj_decoder.bias_hh_l0'])
    return cur + _mlp(sd, 'traj_decoder_out', h), h


def _traj_feat(sd, h):
    return h @ sd['traj_feat_out.weight'].t() + sd['traj_feat_out.bias']


def traj64(sd, trajs, traj_mask, vel_mask, feats, odom, depths, depth_masks, t_out, mask_feats, dtype=torch.float64):
    """The whole trajectory path: encoder GRU, traj_encoder_out, and the t_out decoder steps, whose instance features are taken
    from the SUPPLIED ``mask_feats[:, t]`` [N, 1 + t_out, 256, 14, 14] (not from a ConvLSTM of its own) -> normalized_trajectory,
    unnormalized_trajectory, and the traj_feat_out vectors the ConvLSTM reads: 'enc_tfeat' [N, t_in, 16], 'dec_tfeat' [N, t_out, 16]."""
    d = dtype
    sd = _cast({k: v for k, v in sd.items() if not k.startswith('mask_')}, d)
    odom, enc_h, mean, std = _traj_encode(sd, trajs, traj_mask, vel_mask, feats, odom, depths, depth_masks, d)
    t_in = len(enc_h)
    h = enc_h[-1]
    cur = _mlp(sd, 'traj_encoder_out', h)
    out, dec_tf = [cur], []
    for t in range(t_out):
        cur, h = _traj_step(sd, cur, h, mask_feats[:, t].to(d), odom[:, t_in + t], d)
        out.append(cur)
        dec_tf.append(_traj_feat(sd, h))
    traj = torch.stack(out, 1)
    return {'normalized_trajectory': traj, 'unnormalized_trajectory': traj * std + mean,
            'enc_tfeat': torch.stack([_traj_feat(sd, hh) for hh in enc_h], 1), 'dec_tfeat': torch.stack(dec_tf, 1)}


def gather64(mask_feats, output_inds):
    """output_feats = mask_feats[:, -t_out:][range(N), output_inds] (fg_model.py:334)."""
    n = mask_feats.size(0)
    return mask_feats[:, 1:][torch.arange(n, device=mask_feats.device), output_inds]


def head64(sd, output_feats, classes, dtype=torch.float64, upto=None):
    """mask_fcn1..4 (+ ReLU), deconv (+ ReLU), the predictor row of each instance's class -> masks [N, 28, 28].
    ``upto`` = 'fcn' / 'deconv' returns the activation behind that layer instead."""
    w = lambda k: sd['mask_head.' + k].to(dtype)
    y = output_feats.to(dtype)
    for k in range(1, 5):
        y = F.relu(F.conv2d(y, w('mask_fcn%d.weight' % k), w('mask_fcn%d.bias' % k), padding=1))
    if upto == 'fcn':
        return y
    y = F.relu(F.conv_transpose2d(y, w('deconv.weight'), w('deconv.bias'), stride=2))
    if upto == 'deconv':
        return y
    wp = w('predictor.weight')[classes, :, 0, 0]
    return torch.einsum('nchw,nc->nhw', y, wp) + w('predictor.bias')[classes][:, None, None]


def forward64(sd, trajs, traj_mask, vel_mask, feats, output_inds, odom, depths, depth_masks, classes, t_out, dtype=torch.float64,
              taps=None):
    """FGModel.forward (fg_model.py:216-339) of the shipped config in float64 (or ``dtype``); sd = state_dict.
    ``taps``: a dict that receives 'enc_l0' (layer 0's h of every encoder step), 'cell0_pre' (the four gate pre-activations of
    every layer-0 cell evaluation, encoder then decoder) and 'enc_tfeat' (traj_feat_out of every encoder step)."""
    d = dtype
    dev = trajs.device
    sd = _cast(sd, d)
    feats = feats.to(d)
    odom, enc_h, mean, std = _traj_encode(sd, trajs, traj_mask, vel_mask, feats, odom, depths, depth_masks, d)
    n, t_in = feats.shape[:2]
    h = enc_h[-1]
    z = torch.zeros(n, 256, 14, 14, dtype=d, device=dev)
    h0, c0 = z, z
    l0, pre0 = [], []
    for t in range(t_in):
        h0, c0, pre = cell64(sd, 'mask_encoder.cell_list.0.conv', torch.cat([_plane(_traj_feat(sd, enc_h[t])), feats[:, t]], 1), h0, c0,
                             d, gates=True)
        l0.append(h0)
        pre0.append(pre)
    h1, c1 = z, z
    for t in range(t_in):
        h1, c1 = cell64(sd, 'mask_encoder.cell_list.1.conv', l0[t], h1, c1, d)
    cur = _mlp(sd, 'traj_encoder_out', h)
    cmf = F.conv2d(h1, sd['mask_encoder_out.weight'], sd['mask_encoder_out.bias'])
    trajs_out, mfs = [cur], [cmf]
    for t in range(t_out):
        cur, h = _traj_step(sd, cur, h, cmf, odom[:, t_in + t], d)
        trajs_out.append(cur)
        h0, c0, pre = cell64(sd, 'mask_decoder.cell_list.0.conv', torch.cat([_plane(_traj_feat(sd, h)), cmf], 1), h0, c0, d, gates=True)
        pre0.append(pre)
        h1, c1 = cell64(sd, 'mask_decoder.cell_list.1.conv', h0, h1, c1, d)
        cmf = F.conv2d(h1, sd['mask_decoder_out.weight'], sd['mask_decoder_out.bias'])
        mfs.append(cmf)
    if taps is not None:
        taps.update(enc_l0=l0, cell0_pre=pre0, enc_tfeat=torch.stack([_traj_feat(sd, hh) for hh in enc_h], 1))
    traj = torch.stack(trajs_out, 1)
    mf = torch.stack(mfs, 1)
    of = gather64(mf, output_inds)
    return {'normalized_trajectory': traj, 'unnormalized_trajectory': traj * std + mean, 'mask_feats': mf,
            'output_feats': of, 'masks': head64(sd, of, classes, d)}


# ---------------------------------------------------------------------------------------------- crafted weights
ONEHOT_A = (0, 15, 16, 63, 64, 127, 200, 255)      # first / last / interior columns of the 16-column groups, all four 64-column tiles
ONEHOT_B = (1, 31, 48, 79, 128, 191, 192, 254)
_CELLS = ('mask_encoder.cell_list.0.conv', 'mask_encoder.cell_list.1.conv', 'mask_decoder.cell_list.0.conv',
          'mask_decoder.cell_list.1.conv')


def crafted(sd, which):
    """A copy of the state_dict ``sd`` (the base fill) with a few tensors replaced, so that layers next to the one under test are
    exact identities.  ``which``: one item or a list of items, an item being a name or (name, argument):
      ('ident_fcn', k)            mask_fcn<k>: centre tap = delta(cout, cin), zero bias (behind it: relu(x), exactly)
      'replicate_deconv'          deconv W[cin][cout][dy][dx] = delta(cin, cout) for all four (dy, dx), zero bias
      ('onehot_predictor', chans) predictor row k selects channel chans[k], zero bias
      'ident_out_conv'            mask_encoder_out / mask_decoder_out = identity, zero bias
      'transparent_cell1'         layer 1 of mask_encoder: W_g = identity (centre tap) on the x half, every other weight 0,
                                  b_i = b_o = 20, b_f = b_g = 0: from c = 0, h1 = s(20) tanh(s(20) tanh(x)), s(20) = 1 in fp32
      ('const_traj_feat', scale)  traj_feat_out.weight = 0, bias_k = (-1)^k scale (1 + k/32): the 16 plane-constant channels of
                                  the ConvLSTM input are exactly the bias
      ('hot', gain)               the four ConvLSTM conv weights times gain
    Only the replaced keys are new tensors (``out[k] is not sd[k]``)."""
    items = which if isinstance(which, list) else [which]
    out = dict(sd)
    new = {}
    like = lambda k: dict(dtype=sd[k].dtype, device=sd[k].device)
    eye = lambda k: torch.eye(256, **like(k))
    for item in items:
        name, arg = (item, None) if isinstance(item, str) else item
        if name == 'ident_fcn':
            k = 'mask_head.mask_fcn%d' % arg
            w = torch.zeros_like(sd[k + '.weight'])
            w[:, :, 1, 1] = eye(k + '.weight')
            new[k + '.weight'], new[k + '.bias'] = w, torch.zeros_like(sd[k + '.bias'])
        elif name == 'replicate_deconv':
            k = 'mask_head.deconv'
            new[k + '.weight'] = eye(k + '.weight')[:, :, None, None].expand(-1, -1, 2, 2).contiguous()
            new[k + '.bias'] = torch.zeros_like(sd[k + '.bias'])
        elif name == 'onehot_predictor':
            k = 'mask_head.predictor'
            assert len(arg) == 8
            w = torch.zeros_like(sd[k + '.weight'])
            w[torch.arange(8), torch.as_tensor(arg), 0, 0] = 1
            new[k + '.weight'], new[k + '.bias'] = w, torch.zeros_like(sd[k + '.bias'])
        elif name == 'ident_out_conv':
            for k in ('mask_encoder_out', 'mask_decoder_out'):
                new[k + '.weight'] = eye(k + '.weight')[:, :, None, None].contiguous()
                new[k + '.bias'] = torch.zeros_like(sd[k + '.bias'])
        elif name == 'transparent_cell1':
            k = _CELLS[1]
            w = torch.zeros_like(sd[k + '.weight'])
            w[768:, :256, 1, 1] = eye(k + '.weight')
            b = torch.zeros_like(sd[k + '.bias'])
            b[:256] = 20
            b[512:768] = 20
            new[k + '.weight'], new[k + '.bias'] = w, b
        elif name == 'const_traj_feat':
            k = 'traj_feat_out'
            j = torch.arange(16, **like(k + '.bias'))
            new[k + '.weight'] = torch.zeros_like(sd[k + '.weight'])
            new[k + '.bias'] = (1 - 2 * (j % 2)) * arg * (1 + j / 32)
        elif name == 'hot':
            for k in _CELLS:
                new[k + '.weight'] = sd[k + '.weight'] * arg
        else:
            raise ValueError('crafted: unknown set %r' % (name,))
    out.update(new)
    return out


def saturation(pre, lo=10.0, hi=20.0):
    """(share of the gate pre-activations ``pre`` = (i, f, o, g) beyond +-lo, their largest magnitude): the condition of the
    saturated-regime test is share >= 0.05 and max > hi."""
    v = torch.cat([p.reshape(-1) for p in pre]).abs()
    return float((v > lo).double().mean()), float(v.max())
