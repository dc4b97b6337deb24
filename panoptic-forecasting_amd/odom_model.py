"""``task: odom`` - the odometry forecaster (OdomModel, models/odom/odom_model.py) on libpfhip.so.

The module holds the reference's 8 parameters under the reference's state_dict keys (checkpoints load both ways) and
runs inference through ``pf_odom_forward`` (csrc/odom_net.hip): the whole forecast - normalisation, the T_in - 1 encoder
GRU steps, the T_out decoder steps with the output head and the feedback, unnormalisation - is one kernel launch.  The
parameters are packed into one device buffer by ``pf_odom_pack``; they are packed again whenever a parameter changes
(``load()``, ``load_state_dict``, ``.to()``).

Supported configuration: the shipped odom config (pretrained_models/odom/config.yaml: ``simple_odom``, ``normalize_input``,
``rnn_hidden`` 128, no ``inp_emb_layers`` / ``out_layers``), with ``predict_type`` direct or offset.  Anything else is
refused by ``check_config`` with a ValueError naming the key; training (``loss``) is not built.
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


class OdomModel(BaseModel):
    def __init__(self, params):
        super().__init__()
        check_config(params)
        self.predict_type = params['model']['predict_type']
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

    def predict(self, inputs, labels):
        """OdomModel.predict (odom_model.py:117-121): labels['odometry'] only gives the number of forecast steps."""
        preds, _ = self(inputs['odometry'], labels['odometry'].size(1))
        return {'odometry': preds}
