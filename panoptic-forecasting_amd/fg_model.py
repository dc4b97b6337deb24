"""``task: fg`` - the foreground forecaster (FGModel, models/fg/fg_model.py) on libpfhip.so.

The module holds the reference's 52 parameters under the reference's state_dict keys (checkpoints load both ways) and
runs inference through ``pf_fg_forward`` (csrc/fg_net.hip): ConvLSTM cells and the mask head on fp32 matrix
instructions, the trajectory GRU path on small kernels.  ``model.fg_arithmetic: 'fp16_pair'`` runs the eight 3x3 GEMMs on
the 16-bit matrix instruction with two fp16 terms per fp32 operand instead (PF_FG_PAIR, include/pfhip.h); a forward whose
operands leave the pair's range is then handled as ``model.fg_on_range`` says (see ``FGModel.forward``).  The parameters are packed into one device buffer by
``pf_fg_pack``; they are packed again whenever a parameter changes (``load()``, ``load_state_dict``, ``.to()``).
``predict_panoptic`` / ``predict_semantics`` finish through the existing fg -> panoptic merge (panoptic.PanopticMerger).

Supported configuration: the shipped fg config (pretrained_models/fg/config.yaml).  Every shape switch of the reference
that would change the network is refused in ``__init__`` with a ValueError naming the key; training (``loss``) and
``predict_instances`` are not built.
"""
import ctypes

import torch
from torch import nn

from . import lib as _lib
from .model_api import BaseModel
from .panoptic import PanopticMerger

# (key, value this build computes, reference default when the key is absent)
_FIXED = (('rnn_type', 'gru', None), ('num_convlstm_layers', 2, 1), ('num_traj_out_layers', 2, 1), ('rnn_hidden', 128, None),
          ('instance_feat_channels', 8, None), ('instance_feat_hidden', 64, None), ('traj_feat_channels', 16, None))
_MUST_BE_ON = ('use_odometry', 'use_depth_inp')
_MUST_BE_OFF = ('only_loc_feats', 'no_traj_inst_feats', 'no_mask_traj_feats', 'only_input_odometry')
ODOM_SIZE = 5
T_IN_MAX = T_OUT_MAX = 16
ARITHMETIC_FLAGS = {'fp32': 0, 'fp16_pair': 1}          # include/pfhip.h: PF_FG_PAIR
ON_RANGE = ('rerun', 'raise', 'ignore')
PF_STATUS_RANGE, PF_STATUS_RANGE_LOW = 1, 2             # include/pfhip.h
_STATUS_NAMES = ((PF_STATUS_RANGE, 'PF_STATUS_RANGE (an operand of a 3x3 GEMM exceeded 65504 in magnitude)'),
                 (PF_STATUS_RANGE_LOW, 'PF_STATUS_RANGE_LOW (a K source of a launch had a non-zero maximum below 2^-6)'))


def check_config(params):
    """ValueError naming the first key of ``params`` whose value this build does not compute."""
    model = params['model']
    for key, want, default in _FIXED:
        got = model.get(key, default)
        if got != want:
            raise ValueError('fg: model.%s = %r is not supported (this build computes %r; rnn_type lstm and the other shape '
                             'switches are not built)' % (key, got, want))
    for key in _MUST_BE_ON:
        if not model.get(key):
            raise ValueError('fg: model.%s must be true (the build computes the shipped configuration only)' % key)
    for key in _MUST_BE_OFF:
        if model.get(key):
            raise ValueError('fg: model.%s is not supported (the build computes the shipped configuration only)' % key)
    odom = params.get('data', {}).get('odom_size')
    if odom != ODOM_SIZE:
        raise ValueError('fg: data.odom_size = %r is not supported (this build computes %d)' % (odom, ODOM_SIZE))
    arith = model.get('fg_arithmetic', 'fp32')
    if arith not in ARITHMETIC_FLAGS:
        raise ValueError("fg: model.fg_arithmetic = %r is not supported ('fp32' or 'fp16_pair')" % (arith,))
    on_range = model.get('fg_on_range', 'rerun')
    if on_range not in ON_RANGE:
        raise ValueError("fg: model.fg_on_range = %r is not supported ('rerun', 'raise' or 'ignore')" % (on_range,))


def _norm(params, key, size):
    v = params['data'].get(key)
    if v is None:
        return torch.zeros(1, size), torch.zeros(1, size)
    mean, std = v
    return torch.as_tensor(mean, dtype=torch.float32).reshape(1, size), torch.as_tensor(std, dtype=torch.float32).reshape(1, size)


class _Cell(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.conv = nn.Conv2d(cin + 256, 4 * 256, 3, padding=1)


class _ConvLSTM(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.cell_list = nn.ModuleList([_Cell(cin), _Cell(256)])


class _MaskHead(nn.Module):
    def __init__(self):
        super().__init__()
        for k in range(1, 5):
            self.add_module('mask_fcn%d' % k, nn.Conv2d(256, 256, 3, padding=1))
        self.deconv = nn.ConvTranspose2d(256, 256, 2, stride=2)
        self.predictor = nn.Conv2d(256, 8, 1)


def _mlp():
    return nn.Sequential(nn.Linear(128, 128), nn.ReLU(inplace=True), nn.Linear(128, 10))


class FGModel(BaseModel):
    def __init__(self, params):
        super().__init__()
        check_config(params)
        self.use_bbox_ulbr = params.get('use_bbox_ulbr')
        self.use_depth_sorting = params['model'].get('use_depth_sorting')
        # parameter registration order = the reference's state_dict order (= the raw order pf_fg_pack expects)
        self.odom_mean, self.odom_std = (nn.Parameter(t, requires_grad=False) for t in _norm(params, 'odom_norm_params', 5))
        self.depth_mean, self.depth_std = (nn.Parameter(t, requires_grad=False) for t in _norm(params, 'depth_norm_params', 2))
        self.traj_encoder = nn.GRU(80, 128, batch_first=True)
        self.traj_decoder = nn.GRU(79, 128, batch_first=True)
        self.traj_mean, self.traj_std = (nn.Parameter(t, requires_grad=False) for t in _norm(params, 'norm_params', 8))
        self.traj_encoder_out = _mlp()
        self.traj_decoder_out = _mlp()
        self.traj_feat_out = nn.Linear(128, 16)
        self.instance_compressor = nn.Conv2d(256, 8, 1)
        self.instance_feat_model = nn.Linear(8 * 14 * 14, 64)
        self.mask_encoder = _ConvLSTM(256 + 16)
        self.mask_decoder = _ConvLSTM(256 + 16)
        self.mask_encoder_out = nn.Conv2d(256, 256, 1)
        self.mask_decoder_out = nn.Conv2d(256, 256, 1)
        self.mask_head = _MaskHead()
        self.merger = PanopticMerger(use_depth_sorting=bool(self.use_depth_sorting), use_bbox_ulbr=bool(self.use_bbox_ulbr))
        self.fg_arithmetic = params['model'].get('fg_arithmetic', 'fp32')
        self.fg_on_range = params['model'].get('fg_on_range', 'rerun')
        self._packed = {}          # flags -> (parameter key, packed buffer, raw source kept alive)
        self._ws = {}              # flags -> workspace

    # ---------------------------------------------------------------------------------------------- weights
    def _param_key(self):
        return tuple((t.data_ptr(), t._version) for t in self.state_dict().values())

    @property
    def _flags(self):
        return ARITHMETIC_FLAGS[self.fg_arithmetic]

    def packed_weights(self, flags=None):
        """The device buffer pf_fg_pack filled from the current parameters under ``flags`` (default: those of
        ``fg_arithmetic``); re-packed when any parameter changed.  One buffer per arithmetic is kept."""
        flags = self._flags if flags is None else flags
        key = self._param_key()
        have = self._packed.get(flags)
        if have is not None and have[0] == key:
            return have[1]
        L = _lib.load()
        raw_n, packed_n = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(L.pf_fg_weights_size(flags, ctypes.byref(raw_n), ctypes.byref(packed_n)), 'pf_fg_weights_size')
        sd = self.state_dict()
        dev = next(iter(sd.values())).device
        _lib.require_cuda(torch.empty(0, device=dev), 'FGModel parameters')
        raw = torch.cat([v.detach().reshape(-1).float() for v in sd.values()])
        if raw.numel() != raw_n.value:
            raise _lib.PfError('fg: %d parameter floats, pf_fg_pack expects %d' % (raw.numel(), raw_n.value))
        packed = torch.empty(packed_n.value, dtype=torch.float32, device=dev)
        _lib.check(L.pf_fg_pack(raw.data_ptr(), packed.data_ptr(), flags, _lib.stream_ptr()), 'pf_fg_pack')
        self._packed[flags] = (key, packed, raw)      # pf_fg_pack is asynchronous: its source stays alive until the next pack
        return packed

    def _workspace(self, n, t_in, t_out, device, flags):
        need = ctypes.c_size_t()
        if flags:
            _lib.check(_lib.load().pf_fg_pair_workspace(n, t_in, t_out, ctypes.byref(need)), 'pf_fg_pair_workspace')
        else:
            _lib.check(_lib.load().pf_fg_workspace(n, t_in, t_out, 0, ctypes.byref(need)), 'pf_fg_workspace')
        ws = self._ws.get(flags)
        if ws is None or ws.numel() < need.value or ws.device != device:
            ws = self._ws[flags] = torch.empty(max(need.value, 1), dtype=torch.uint8, device=device)
            if flags:                   # the status block in front of a pair workspace is cleared once, by its owner
                _lib.check(_lib.load().pf_fg_status_reset(ws.data_ptr(), _lib.stream_ptr()), 'pf_fg_status_reset')
        return ws

    def _read_status(self, ws):
        out2 = (ctypes.c_uint * 2)()
        _lib.check(_lib.load().pf_fg_status(ws.data_ptr(), out2, _lib.stream_ptr()), 'pf_fg_status')
        return int(out2[0]), int(out2[1])

    def fg_status(self):
        """PF_STATUS_* bits of every 'fp16_pair' forward since the last read, then cleared (synchronises; 0 in 'fp32' mode).
        ``forward`` cannot read the status while a stream capture records it: read it here after the replays.  The words live in
        the model's pair workspace: a forward of more instances or steps than any before allocates a new one with clear words."""
        ws = self._ws.get(self._flags) if self._flags else None
        if ws is None:
            return 0
        last, sticky = self._read_status(ws)
        return last | sticky

    # ---------------------------------------------------------------------------------------------- forward
    @torch.no_grad()
    def forward(self, input_trajs, traj_mask, traj_vel_mask, instance_feats, output_inds, odom, input_depths,
                input_depth_masks, classes, num_output_steps):
        """FGModel.forward (fg_model.py:216-339): same arguments, same dict.

        ``fg_arithmetic == 'fp16_pair'``: after the enqueue the two status words are read with ONE synchronisation; when
        PF_STATUS_RANGE / PF_STATUS_RANGE_LOW is set, ``fg_on_range`` decides: 'rerun' (default) runs the same forward again
        with flags = 0 into the same output tensors (then bit-identical to the 'fp32' mode), 'raise' raises PfError naming
        the bit, 'ignore' returns what the pair path computed.  While the stream is being captured nothing can be read:
        the forward is enqueued only and the caller reads ``fg_status()`` after the replays.  'fp32' never synchronises."""
        flags = self._flags
        packed = self.packed_weights()
        dev = packed.device
        n, t_in = input_trajs.shape[0], input_trajs.shape[1]
        t_out = int(num_output_steps)
        if not (1 <= t_in <= T_IN_MAX and 1 <= t_out <= T_OUT_MAX):
            raise ValueError('fg: %d input / %d output steps (1..16 each are built)' % (t_in, t_out))
        f32 = lambda t, shape, name: _lib.require_cuda(t.to(dev, torch.float32).reshape(shape).contiguous(), name)
        i64 = lambda t, name: _lib.require_cuda(torch.as_tensor(t).to(dev, torch.int64).reshape(n).contiguous(), name)
        odom_t = odom.shape[1]
        args = (f32(input_trajs, (n, t_in, 8), 'input_trajs'), f32(traj_mask[:, :t_in], (n, t_in), 'traj_mask'),
                f32(traj_vel_mask[:, :t_in], (n, t_in), 'traj_vel_mask'),
                f32(instance_feats, (n, t_in, 256, 14, 14), 'instance_feats'), i64(output_inds, 'output_inds'),
                f32(odom, (n, odom_t, ODOM_SIZE), 'odom'), f32(input_depths, (n, t_in, 2), 'input_depths'),
                f32(input_depth_masks, (n, t_in), 'input_depth_masks'), i64(classes, 'classes'))
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        out = {'normalized_trajectory': new(n, 1 + t_out, 10), 'unnormalized_trajectory': new(n, 1 + t_out, 10),
               'mask_feats': new(n, 1 + t_out, 256, 14, 14), 'output_feats': new(n, 256, 14, 14), 'masks': new(n, 28, 28)}

        def run(fl):
            # a PF_FG_PAIR buffer holds the flags = 0 layout in front of its pair section: the re-run needs no second pack
            ws = self._workspace(n, t_in, t_out, dev, fl)
            rc = _lib.load().pf_fg_forward(packed.data_ptr(), fl, n, t_in, t_out, odom_t, *[a.data_ptr() for a in args],
                                           *[out[k].data_ptr() for k in ('normalized_trajectory', 'unnormalized_trajectory',
                                                                         'mask_feats', 'output_feats', 'masks')],
                                           ws.data_ptr(), ws.numel(), _lib.stream_ptr())
            _lib.check(rc, 'pf_fg_forward')
            return ws

        ws = run(flags)
        if flags and n and self.fg_on_range != 'ignore' and not torch.cuda.is_current_stream_capturing():
            status, _ = self._read_status(ws)
            if status & (PF_STATUS_RANGE | PF_STATUS_RANGE_LOW):
                if self.fg_on_range == 'raise':
                    raise _lib.PfError("fg forward (model.fg_arithmetic = 'fp16_pair'): status %d: %s; run with model.fg_arithmetic "
                                       "= 'fp32' or model.fg_on_range = 'rerun'"
                                       % (status, ', '.join(name for bit, name in _STATUS_NAMES if status & bit)))
                run(0)
        return out

    # ---------------------------------------------------------------------------------------------- predict
    def _predict(self, inputs, labels, panoptic):
        dev = next(iter(self.state_dict().values())).device
        cat = lambda key: torch.cat([x.to(dev) for x in inputs[key]])
        counts = [len(x) for x in inputs['feats']]
        trajs = cat('trajectories')
        t_in = trajs.size(1)
        out_t = labels['trajectories'][0].size(1)
        output_inds = torch.cat([x.to(dev) for x in labels['output_inds']])
        classes = [c.to(dev) for c in inputs['classes']]
        pred = self(trajs, cat('bbox_masks').float()[:, :t_in], cat('bbox_vel_masks').float()[:, :t_in], cat('feats'),
                    output_inds, cat('odometry'), cat('depths'), cat('depth_masks'), torch.cat(classes), out_t)
        traj = pred['unnormalized_trajectory'][:, -out_t:]                                         # :534
        idx = torch.arange(traj.size(0), device=dev)
        boxes = traj[idx, output_inds, :4]                                                         # :538
        depths = traj[idx, output_inds, 8]                                                         # :545
        to_dev = lambda key: None if inputs.get(key) is None else [x.to(dev) for x in inputs[key]]
        seg = self.merger.predict_panoptic({'masks': pred['masks'], 'boxes': boxes, 'depths': depths}, classes,
                                           to_dev('background'), to_dev('background_depth'), to_dev('background_depth_mask'),
                                           panoptic=panoptic)['seg']
        return {'seg': seg, 'bbox': traj[:, :, :4].split(counts), 'depths': traj[:, :, 8].split(counts)}

    def predict_panoptic(self, inputs, labels):
        """FGModel.predict_panoptic (fg_model.py:489-595): seg [B,1024,2048] with (class+11)*1000 + id, bbox, depths."""
        return self._predict(inputs, labels, True)

    def predict_semantics(self, inputs, labels):
        """FGModel.predict_semantics (fg_model.py:389-487): seg with class+11 values over the untouched background."""
        return self._predict(inputs, labels, False)
