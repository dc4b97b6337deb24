"""Test helper for fg training (not a test module): the reference's loss (fg_model.py:341-387, losses.py:34-189, shipped
config: smoothl1, supervise_last_inp, depth input on) restated functionally on top of ``fg_ref64.forward64``, in any dtype
and on any device, and the counter-based training batch of the fixture.  tests/test_fg_train_host.py pins ``loss64`` and
its autograd gradients to the reference's own float64 run in g11_fgtrain.npz.  Nothing native uses it yet.
"""
import numpy as np
import torch
import torch.nn.functional as F

import fg_ref64 as R

LOSS_KEYS = ('traj_2d_loss', 'center_pixel_l2', 'center_pixel_fde', 'size_pixel_l1', 'depth_l2', 'mask_distill_loss', 'loss')
NORM_KEYS = ('odom_mean', 'odom_std', 'depth_mean', 'depth_std', 'traj_mean', 'traj_std')
CELL_KEYS = tuple('mask_%s.cell_list.%d.conv.%s' % (m, l, w) for m in ('encoder', 'decoder') for l in (0, 1)
                  for w in ('weight', 'bias'))
SAMPLES = 4096            # the fixture stores tensors with more elements as this many seeded samples


def is_trained(key):
    return key not in NORM_KEYS and not key.startswith('mask_head.')


def sample_index(key_number, numel):
    """The fixture's sample positions of a tensor (sorted flat indices)."""
    return np.sort(np.random.RandomState(1100 + key_number).choice(numel, SAMPLES, replace=False)).astype(np.int64)


def make_batch(case, counts, t_out=3, output_inds=None, holes=True):
    """(inputs, labels) as the fg_instance collate hands them to ``loss``: tensors over all N instances, ``bbox_masks`` /
    ``bbox_vel_masks`` / ``feat_masks`` of length T_in + t_out.  The input half is ``fg_ref64.make_inputs``; labels and the
    output half of the masks come from streams 1900 + 100*case + j.  Holes (where N allows): feat_masks[1,0], [3,2], [2,4],
    bbox_masks[2, T_in + t_out - 1], label depth_masks[0, t_out - 1]."""
    lists, lab = R.make_inputs(case, counts, t_out=t_out, output_inds=output_inds)
    n = int(sum(counts))
    t_in = R.T_IN
    base = 1900 + 100 * case
    u = lambda j, shape: torch.from_numpy(R.uniform(base + j, int(np.prod(shape))).astype(np.float32).reshape(shape))
    inputs = {k: torch.cat(v) for k, v in lists.items()}
    fm = torch.ones(n, t_in + t_out)
    bm = torch.ones(n, t_in + t_out)
    bm[:, :t_in] = inputs['bbox_masks'].float()
    ldm = torch.ones(n, t_out, 1, dtype=torch.bool)
    if holes:
        if n > 1:
            fm[1, 0] = 0
        if n > 3:
            fm[3, 2] = 0
        if n > 2:
            fm[2, min(4, t_in + t_out - 1)] = 0
            bm[2, t_in + t_out - 1] = 0
        if n > 0:
            ldm[0, t_out - 1, 0] = False
    vm = torch.zeros(n, t_in + t_out)
    vm[:, 1:] = bm[:, 1:] * bm[:, :-1]
    inputs['feat_masks'] = fm
    inputs['bbox_masks'], inputs['bbox_vel_masks'] = bm.bool(), vm.bool()
    labels = {'trajectories': torch.tensor(R.TRAJ_MEAN) + torch.tensor(R.TRAJ_STD) * (2 * u(0, (n, t_out, 8)) - 1),
              'depths': torch.tensor(R.DEPTH_MEAN) + torch.tensor(R.DEPTH_STD) * (2 * u(1, (n, t_out, 2)) - 1),
              'depth_masks': ldm, 'feats': u(2, (n, t_out, 256, 14, 14)), 'output_inds': torch.cat(lab['output_inds'])}
    return inputs, labels


def to_device(d, dev):
    return {k: v.to(dev) for k, v in d.items()}


def _pairs(mask):
    """expand_traj_mask's velocity half: a step counts when it and its predecessor are present."""
    return torch.cat([torch.zeros_like(mask[:, :1]), mask[:, 1:] * mask[:, :-1]], 1)


def _cwh(b):
    return torch.stack([(b[..., 0] + b[..., 2]) / 2, (b[..., 1] + b[..., 3]) / 2, b[..., 2] - b[..., 0], b[..., 3] - b[..., 1]], -1)


def loss_terms(pred_unnorm, pred_feats, inputs, labels, dtype, use_bbox_ulbr=False, traj_coef=0.1, mask_distill_coef=1.0):
    """The seven [N] loss tensors from the network's two outputs (any dtype / device)."""
    d = dtype
    t_out = labels['trajectories'].size(1)
    keep = t_out + 1
    f = lambda t: t.to(pred_unnorm.device, d)
    bm = f(inputs['bbox_masks'])[:, -keep:]
    vm = f(inputs['bbox_vel_masks'])[:, -keep:]
    dm_all = torch.cat([f(inputs['depth_masks']), f(labels['depth_masks'])], 1).squeeze(-1)
    dm, dvm = dm_all[:, -keep:], _pairs(dm_all)[:, -keep:]
    gt_box = torch.cat([f(inputs['trajectories'])[:, -1:], f(labels['trajectories'])], 1)
    gt_depth = torch.cat([f(inputs['depths'])[:, -1:], f(labels['depths'])], 1)
    gt = torch.cat([gt_box, gt_depth], -1)
    w = torch.cat([bm[..., None].expand(-1, -1, 4), vm[..., None].expand(-1, -1, 4), dm[..., None], dvm[..., None]], -1)
    # the reference keeps the 0/1 box and depth masks in fp32 whatever the model's dtype, so "+ 1e-8" is an fp32 addition
    den = lambda mask: (mask.float().flatten(1).sum(1) + 1e-8).to(d)
    out = {}
    out['traj_2d_loss'] = (F.smooth_l1_loss(pred_unnorm, gt, reduction='none') * w).flatten(1).sum(1) / den(w)
    pb, gb = pred_unnorm[..., :4], gt[..., :4]
    if use_bbox_ulbr:
        pb, gb = _cwh(pb), _cwh(gb)
    centre = torch.norm(pb[..., :2] - gb[..., :2], dim=-1)
    out['center_pixel_l2'] = (centre * bm).sum(1) / den(bm)
    out['center_pixel_fde'] = centre[:, -1] * bm[:, -1]
    out['size_pixel_l1'] = ((pb[..., 2:4] - gb[..., 2:4]).abs() * bm[..., None]).flatten(1).sum(1) / den(bm)
    div = dm.sum(1)
    div = torch.where(div == 0, torch.ones_like(div), div)
    out['depth_l2'] = (torch.norm(pred_unnorm[..., 8:9] - gt_depth[..., 0:1], dim=-1) * dm).sum(1) / div
    fm = f(inputs['feat_masks'])[:, -keep:]
    target = torch.cat([f(inputs['feats'])[:, -1:], f(labels['feats'])], 1)
    per_step = ((pred_feats - target) ** 2).flatten(2).sum(2) * fm
    out['mask_distill_loss'] = per_step.sum(1) / (fm.sum(1) * pred_feats[0, 0].numel() + 1e-8)
    out['loss'] = traj_coef * out['traj_2d_loss'] + mask_distill_coef * out['mask_distill_loss']
    return out


def loss64(sd, inputs, labels, dtype=torch.float64, use_bbox_ulbr=False):
    """FGModel.loss of the shipped config in ``dtype``: {name: [N]} for the seven names of LOSS_KEYS."""
    t_in = inputs['trajectories'].size(1)
    t_out = labels['trajectories'].size(1)
    pred = R.forward64(sd, inputs['trajectories'], inputs['bbox_masks'].float()[:, :t_in], inputs['bbox_vel_masks'].float()[:, :t_in],
                       inputs['feats'], labels['output_inds'], inputs['odometry'], inputs['depths'], inputs['depth_masks'],
                       inputs['classes'], t_out, dtype)
    return loss_terms(pred['unnormalized_trajectory'], pred['mask_feats'], inputs, labels, dtype, use_bbox_ulbr)


def loss_and_grads(sd, inputs, labels, dtype=torch.float64, use_bbox_ulbr=False):
    """({name: [N]}, {key: d loss.mean() / d key or None}) in ``dtype``, for every state_dict key."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(k not in NORM_KEYS) for k, v in sd.items()}
    out = loss64(leaves, inputs, labels, dtype, use_bbox_ulbr)
    keys = [k for k in leaves if k not in NORM_KEYS]
    grads = torch.autograd.grad(out['loss'].mean(), [leaves[k] for k in keys], allow_unused=True)
    g = dict(zip(keys, grads))
    g.update({k: None for k in NORM_KEYS})
    return {k: v.detach() for k, v in out.items()}, g
