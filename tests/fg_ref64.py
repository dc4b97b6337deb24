"""Test helper for the fg forecaster (not a test module): deterministic fills and a float64 functional checker.

Fills are counter-based, so the generator (tests/golden/make_golden_fgnet.py) and the tests rebuild the same weights and
inputs bit for bit without storing them:  u(s, i) = mix32(i * 0x9E3779B1 + (s + 1) * 0x85EBCA77) / 2^32  in [0, 1), where
mix32 is the murmur3 finaliser (x ^= x>>16; x *= 0x85EBCA6B; x ^= x>>13; x *= 0xC2B2AE35; x ^= x>>16, all mod 2^32),
``s`` the stream (the index of the state_dict key, or 1000 + 100*case + input number) and ``i`` the flat element index.

``forward64`` restates FGModel.forward in functional torch ops (conv2d / conv_transpose2d / matmul) for the supported
configuration (the shipped fg config); tests/test_fg_host.py pins it to the reference's own float64 run in the fixture.
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


def make_inputs(case, counts, t_out=3, odom_t=None, output_inds=None, masked=True):
    """Per-image lists (the reference's predict_* inputs) for ``counts`` instances; stream 1000 + 100*case + j."""
    n = int(sum(counts))
    odom_t = odom_t or T_IN + t_out
    base = 1000 + 100 * case
    u = lambda j, shape: torch.from_numpy(uniform(base + j, int(np.prod(shape))).astype(np.float32).reshape(shape))
    mean = torch.tensor(TRAJ_MEAN)
    std = torch.tensor(TRAJ_STD)
    trajs = mean + std * (2 * u(0, (n, T_IN, 8)) - 1)
    depths = torch.tensor(DEPTH_MEAN) + torch.tensor(DEPTH_STD) * (2 * u(1, (n, T_IN, 2)) - 1)
    odom = torch.tensor(ODOM_MEAN) + torch.tensor(ODOM_STD) * (2 * u(2, (n, odom_t, ODOM)) - 1)
    feats = u(3, (n, T_IN, 256, 14, 14))
    mask = torch.ones(n, T_IN)
    dmask = torch.ones(n, T_IN, 1, dtype=torch.bool)
    if masked and n > 1:
        mask[1, 0] = 0                      # instance 1 is missing at the first input step
        dmask[1, 1, 0] = False              # ... and has no depth at the second
    if masked and n > 3:
        mask[3, 2] = 0                      # instance 3 is missing at the most recent input step
    vel = torch.zeros(n, T_IN)
    vel[:, 1:] = mask[:, 1:] * mask[:, :-1]
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


def _cell(sd, pre, x, h, c):
    g = F.conv2d(torch.cat([x, h], 1), sd[pre + '.weight'], sd[pre + '.bias'], padding=1)
    i, f, o, gg = g.chunk(4, 1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
    return torch.sigmoid(o) * torch.tanh(c), c


def _inst_feat(sd, feats):
    x = F.conv2d(feats, sd['instance_compressor.weight'], sd['instance_compressor.bias'])
    x = F.relu(x.reshape(x.size(0), -1))
    return x @ sd['instance_feat_model.weight'].t() + sd['instance_feat_model.bias']


def forward64(sd, trajs, traj_mask, vel_mask, feats, output_inds, odom, depths, depth_masks, classes, t_out, dtype=torch.float64):
    """FGModel.forward (fg_model.py:216-339) of the shipped config in float64 (or ``dtype``); sd = state_dict."""
    d = dtype
    dev = trajs.device
    sd = {k: v.to(d) for k, v in sd.items()}
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
        inst = _inst_feat(sd, feats[:, t]) * m[:, t:t + 1]
        h = _gru(torch.cat([x[:, t], inst, m[:, t:t + 1], odom[:, t]], -1), h, sd['traj_encoder.weight_ih_l0'],
                 sd['traj_encoder.weight_hh_l0'], sd['traj_encoder.bias_ih_l0'], sd['traj_encoder.bias_hh_l0'])
        enc_h.append(h)
    tf = lambda hh: hh @ sd['traj_feat_out.weight'].t() + sd['traj_feat_out.bias']
    plane = lambda v: v[:, :, None, None].expand(-1, -1, 14, 14)
    z = torch.zeros(n, 256, 14, 14, dtype=d, device=dev)
    h0, c0 = z, z
    l0 = []
    for t in range(t_in):
        h0, c0 = _cell(sd, 'mask_encoder.cell_list.0.conv', torch.cat([plane(tf(enc_h[t])), feats[:, t]], 1), h0, c0)
        l0.append(h0)
    h1, c1 = z, z
    for t in range(t_in):
        h1, c1 = _cell(sd, 'mask_encoder.cell_list.1.conv', l0[t], h1, c1)
    cur = _mlp(sd, 'traj_encoder_out', h)
    cmf = F.conv2d(h1, sd['mask_encoder_out.weight'], sd['mask_encoder_out.bias'])
    trajs_out, mfs = [cur], [cmf]
    for t in range(t_out):
        inst = _inst_feat(sd, cmf)
        h = _gru(torch.cat([cur, inst, odom[:, t_in + t]], -1), h, sd['traj_decoder.weight_ih_l0'],
                 sd['traj_decoder.weight_hh_l0'], sd['traj_decoder.bias_ih_l0'], sd['traj_decoder.bias_hh_l0'])
        cur = cur + _mlp(sd, 'traj_decoder_out', h)
        trajs_out.append(cur)
        h0, c0 = _cell(sd, 'mask_decoder.cell_list.0.conv', torch.cat([plane(tf(h)), cmf], 1), h0, c0)
        h1, c1 = _cell(sd, 'mask_decoder.cell_list.1.conv', h0, h1, c1)
        cmf = F.conv2d(h1, sd['mask_decoder_out.weight'], sd['mask_decoder_out.bias'])
        mfs.append(cmf)
    traj = torch.stack(trajs_out, 1)
    mf = torch.stack(mfs, 1)
    of = mf[:, 1:][torch.arange(n, device=dev), output_inds]
    y = of
    for k in range(1, 5):
        y = F.relu(F.conv2d(y, sd['mask_head.mask_fcn%d.weight' % k], sd['mask_head.mask_fcn%d.bias' % k], padding=1))
    y = F.relu(F.conv_transpose2d(y, sd['mask_head.deconv.weight'], sd['mask_head.deconv.bias'], stride=2))
    wp = sd['mask_head.predictor.weight'][classes, :, 0, 0]
    masks = torch.einsum('nchw,nc->nhw', y, wp) + sd['mask_head.predictor.bias'][classes][:, None, None]
    return {'normalized_trajectory': traj, 'unnormalized_trajectory': traj * std + mean, 'mask_feats': mf,
            'output_feats': of, 'masks': masks}
