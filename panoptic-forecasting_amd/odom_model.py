"""``task: odom`` - the odometry forecaster (OdomModel, models/odom/odom_model.py) on libpfhip.so.

The module holds the reference's 8 parameters under the reference's state_dict keys (checkpoints load both ways) and
runs inference through ``pf_odom_forward`` (csrc/odom_net.hip): the whole forecast - normalisation, the T_in - 1 encoder
GRU steps, the T_out decoder steps with the output head and the feedback, unnormalisation - is one kernel launch.  The
parameters are packed into one device buffer by ``pf_odom_pack``; they are packed again whenever a parameter changes
(``load()``, ``load_state_dict``, ``.to()``, an optimiser step).

Training: ``loss`` is the reference's (odom_model.py:104-115) in torch ops on the two outputs of ``forward_train``, an
``autograd.Function`` whose forward is ``pf_odom_train_forward`` (the inference kernel's bits, plus the gates it keeps in a
workspace) and whose backward is ``pf_odom_backward`` (csrc/odom_train.hip: back-propagation through time + the weight
gradients, no atomics).  The optimiser is ``torch.optim`` (train_odom.py).

Supported configuration: the shipped odom config (pretrained_models/odom/config.yaml: ``simple_odom``, ``normalize_input``,
``rnn_hidden`` 128, no ``inp_emb_layers`` / ``out_layers``), with ``predict_type`` direct or offset.  Anything else is
refused by ``check_config`` with a ValueError naming the key.
"""
import ctypes

import torch
from torch import nn

from . import lib as _lib
from .model_api import BaseModel

HIDDEN = 128
ODOM_SIZE = 2               # [speed, yaw_rate]
T_IN_MAX = T_OUT_MAX = 64   # pf_odom_forward's limits
PREDICT_TYPES = ('direct', 'offset')
LOSS_FNS = ('mse', 'smooth_l1')


def check_config(params):
    """ValueError naming the first key of ``params['model']`` whose value this build does not compute."""
    model = params['model']
    if model.get('model_type') != 'simple_odom':
        raise ValueError('odom: model.model_type = %r is outside the odom forecaster of this build (it computes simple_odom, '
                         'the model of every reference odom config)' % (model.get('model_type'),))
    if model.get('predict_type') not in PREDICT_TYPES:
        raise ValueError('odom: model.predict_type = %r is not recognized (direct or offset)' % (model.get('predict_type'),))
    if not model.get('normalize_input'):
        raise ValueError('odom: model.normalize_input must be true (the reference fails in forward without it)')
    if model.get('rnn_hidden') != HIDDEN:
        raise ValueError('odom: model.rnn_hidden = %r is not supported (this build computes %d)' % (model.get('rnn_hidden'), HIDDEN))
    for key in ('inp_emb_layers', 'out_layers'):
        if model.get(key):
            raise ValueError('odom: model.%s = %r is not supported (the build computes the shipped configuration only)'
                             % (key, model[key]))
    if model.get('loss_fn') not in LOSS_FNS:
        raise ValueError('odom: model.loss_fn = %r is not recognized (mse or smooth_l1)' % (model.get('loss_fn'),))


def _norm(params):
    v = params.get('data', {}).get('odom_norm_params')
    if v is None:                      # odom_model.py:20-22: the checkpoint supplies the real values
        return torch.zeros(1, ODOM_SIZE), torch.zeros(1, ODOM_SIZE)
    mean, std = v
    return (torch.as_tensor(mean, dtype=torch.float32).reshape(1, ODOM_SIZE),
            torch.as_tensor(std, dtype=torch.float32).reshape(1, ODOM_SIZE))


class OdomTrainFunction(torch.autograd.Function):
    """(results, normalized_results) = forward(model, inps, t_out, *state_dict tensors): the 8 tensors are arguments only so
    that autograd routes their gradients; the kernels read the packed copy of the same values."""

    @staticmethod
    def forward(ctx, model, inps, t_out, *params):
        L = _lib.load()
        packed = model.packed_weights()
        dev = packed.device
        b, t_in = inps.shape[0], inps.shape[1]
        flags = 1 if model.predict_type == 'offset' else 0
        ws, token = model._train_workspace(b, t_in, t_out, flags)
        results = torch.empty(b, t_out, ODOM_SIZE, dtype=torch.float32, device=dev)
        normalized = torch.empty_like(results)
        _lib.check(L.pf_odom_train_forward(packed.data_ptr(), flags, b, t_in, t_out, inps.data_ptr(), results.data_ptr(),
                                           normalized.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
                   'pf_odom_train_forward')
        ctx.model, ctx.packed, ctx.inps, ctx.normalized, ctx.ws, ctx.token = model, packed, inps, normalized, ws, token
        ctx.dims = (flags, b, t_in, t_out)
        ctx.shapes = [p.shape for p in params]
        ctx.set_materialize_grads(False)
        return results, normalized

    @staticmethod
    def backward(ctx, g_results, g_normalized):
        flags, b, t_in, t_out = ctx.dims
        model, ws = ctx.model, ctx.ws
        key = (b, t_in, t_out)
        if model._ws_token.get(key) is not ctx.token:
            raise RuntimeError('odom: the saved state of this forward_train is gone (a later forward_train of the same shape '
                               'reused the workspace, or this graph was already back-propagated): run one backward per '
                               'forward_train')
        model._ws_token[key] = None            # pf_odom_backward consumes the saved gates
        dev = ctx.packed.device
        ptr = lambda g: None if g is None else g.data_ptr()
        g_results = None if g_results is None else g_results.to(torch.float32).contiguous()
        g_normalized = None if g_normalized is None else g_normalized.to(torch.float32).contiguous()
        grad_raw = torch.empty(sum(s.numel() for s in ctx.shapes), dtype=torch.float32, device=dev)
        _lib.check(_lib.load().pf_odom_backward(ctx.packed.data_ptr(), flags, b, t_in, t_out, ctx.inps.data_ptr(),
                                                ctx.normalized.data_ptr(), ptr(g_results), ptr(g_normalized), ws.data_ptr(),
                                                ws.numel(), grad_raw.data_ptr(), _lib.stream_ptr()), 'pf_odom_backward')
        grads, at = [], 0
        for i, shape in enumerate(ctx.shapes):
            n = shape.numel()
            # odom_mean / odom_std (the first two) never receive a gradient (requires_grad=False in the reference)
            grads.append(grad_raw[at:at + n].view(shape) if i >= 2 and ctx.needs_input_grad[3 + i] else None)
            at += n
        return (None, None, None) + tuple(grads)


class OdomModel(BaseModel):
    def __init__(self, params):
        super().__init__()
        check_config(params)
        self.predict_type = params['model']['predict_type']
        self.use_normalized_loss = params['model'].get('use_normalized_loss')
        self.loss_fn = (nn.SmoothL1Loss if params['model']['loss_fn'] == 'smooth_l1' else nn.MSELoss)(reduction='none')
        self._ws = {}           # (B, T_in, T_out) -> pf_odom_train_workspace bytes on the device
        self._ws_token = {}     # (B, T_in, T_out) -> the forward_train whose state the workspace holds (None: consumed)
        # parameter registration order = the reference's state_dict order (= the raw order pf_odom_pack expects)
        self.odom_mean, self.odom_std = (nn.Parameter(t, requires_grad=False) for t in _norm(params))
        self.rnn = nn.GRU(ODOM_SIZE, HIDDEN, batch_first=True)
        self.out = nn.Sequential(nn.Linear(HIDDEN, ODOM_SIZE))
        self._packed = None
        self._packed_key = None
        self._raw_keepalive = None

    # ---------------------------------------------------------------------------------------------- weights
    def _param_key(self):
        return tuple((t.data_ptr(), t._version) for t in self.state_dict().values())

    def packed_weights(self):
        """The device buffer pf_odom_pack filled from the current parameters (re-packed when any of them changed)."""
        key = self._param_key()
        if self._packed is not None and key == self._packed_key:
            return self._packed
        L = _lib.load()
        raw_n, packed_n = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(L.pf_odom_weights_size(0, ctypes.byref(raw_n), ctypes.byref(packed_n)), 'pf_odom_weights_size')
        sd = self.state_dict()
        dev = next(iter(sd.values())).device
        _lib.require_cuda(torch.empty(0, device=dev), 'OdomModel parameters')
        raw = torch.cat([v.detach().reshape(-1).float() for v in sd.values()])
        if raw.numel() != raw_n.value:
            raise _lib.PfError('odom: %d parameter floats, pf_odom_pack expects %d' % (raw.numel(), raw_n.value))
        packed = torch.empty(packed_n.value, dtype=torch.float32, device=dev)
        _lib.check(L.pf_odom_pack(raw.data_ptr(), packed.data_ptr(), 0, _lib.stream_ptr()), 'pf_odom_pack')
        self._raw_keepalive = raw      # pf_odom_pack is asynchronous: keep its source alive until the next pack
        self._packed, self._packed_key = packed, key
        return packed

    # ---------------------------------------------------------------------------------------------- forward
    @torch.no_grad()
    def forward(self, inps, output_len):
        """OdomModel.forward (odom_model.py:79-106): inps [B,T_in,2] -> (results, normalized_results), each [B,output_len,2]."""
        packed = self.packed_weights()
        dev = packed.device
        if inps.dim() != 3 or inps.size(2) != ODOM_SIZE:
            raise ValueError('odom: inps must be [B, T_in, 2], got %s' % (tuple(inps.shape),))
        b, t_in = inps.shape[0], inps.shape[1]
        t_out = int(output_len)
        if not (2 <= t_in <= T_IN_MAX and 1 <= t_out <= T_OUT_MAX):
            raise ValueError('odom: %d input / %d output steps (2..64 input and 1..64 output steps are built)' % (t_in, t_out))
        x = _lib.require_cuda(inps.to(dev, torch.float32).contiguous(), 'inps')
        results = torch.empty(b, t_out, ODOM_SIZE, dtype=torch.float32, device=dev)
        normalized = torch.empty_like(results)
        flags = 1 if self.predict_type == 'offset' else 0
        _lib.check(_lib.load().pf_odom_forward(packed.data_ptr(), flags, b, t_in, t_out, x.data_ptr(), results.data_ptr(),
                                               normalized.data_ptr(), _lib.stream_ptr()), 'pf_odom_forward')
        return results, normalized

    # ---------------------------------------------------------------------------------------------- training
    def _train_workspace(self, b, t_in, t_out, flags):
        key = (b, t_in, t_out)
        ws = self._ws.get(key)
        dev = self.packed_weights().device
        if ws is None or ws.device != dev:
            n = ctypes.c_size_t()
            _lib.check(_lib.load().pf_odom_train_workspace(b, t_in, t_out, flags, ctypes.byref(n)), 'pf_odom_train_workspace')
            ws = self._ws[key] = torch.empty(n.value, dtype=torch.uint8, device=dev)
        token = self._ws_token[key] = object()
        return ws, token

    def forward_train(self, inps, output_len):
        """``forward`` with a grad_fn: the same (results, normalized_results) bit for bit, differentiable with respect to the
        six trainable tensors (not ``inps``).  One ``backward`` per call: the saved state lives in a workspace cached per
        (B, T_in, output_len), which the next ``forward_train`` of that shape reuses."""
        packed = self.packed_weights()
        dev = packed.device
        if inps.dim() != 3 or inps.size(2) != ODOM_SIZE:
            raise ValueError('odom: inps must be [B, T_in, 2], got %s' % (tuple(inps.shape),))
        if inps.requires_grad:
            raise ValueError('odom: inps.requires_grad is set: no gradient is produced for the input odometry')
        t_in, t_out = inps.shape[1], int(output_len)
        if not (2 <= t_in <= T_IN_MAX and 1 <= t_out <= T_OUT_MAX):
            raise ValueError('odom: %d input / %d output steps (2..64 input and 1..64 output steps are built)' % (t_in, t_out))
        x = _lib.require_cuda(inps.to(dev, torch.float32).contiguous(), 'inps')
        return OdomTrainFunction.apply(self, x, t_out, *self._state_tensors())

    def _state_tensors(self):
        """The 8 tensors in state_dict order, as the Parameters themselves (state_dict() detaches)."""
        return [self.odom_mean, self.odom_std, self.rnn.weight_ih_l0, self.rnn.weight_hh_l0, self.rnn.bias_ih_l0,
                self.rnn.bias_hh_l0, self.out[0].weight, self.out[0].bias]

    def loss(self, inputs, labels):
        """OdomModel.loss (odom_model.py:104-115): {'loss': [B]}, the per-sequence mean of the element-wise loss."""
        if not self.odom_mean.is_cuda:          # before anything is read: the library has no CPU path (lib.py)
            raise NotImplementedError('OdomModel.loss needs the parameters on a GPU (libpfhip.so has no CPU path)')
        inp_odom, label_odom = inputs['odometry'], labels['odometry']
        # under no_grad (validation) nothing is saved: the inference launch gives the same bits
        run = self.forward_train if torch.is_grad_enabled() else self
        preds, normalized_preds = run(inp_odom, label_odom.size(1))
        label_odom = label_odom.to(preds.device, torch.float32)
        if self.use_normalized_loss:
            normalized_label = (label_odom - self.odom_mean.detach()) / self.odom_std.detach()
            loss = self.loss_fn(normalized_preds, normalized_label)
        else:
            loss = self.loss_fn(preds, label_odom)
        return {'loss': loss.flatten(1).mean(1)}       # flatten, not reshape(B, -1): B = 0 leaves -1 ambiguous

    def predict(self, inputs, labels):
        """OdomModel.predict (odom_model.py:117-121): labels['odometry'] only gives the number of forecast steps."""
        preds, _ = self(inputs['odometry'], labels['odometry'].size(1))
        return {'odometry': preds}
