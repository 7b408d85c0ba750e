"""WorldModelProbe(model='gru_probe'): the supervised baseline the probe numbers are read against (reference:
pydreamer/models/baselines.py:19-111 WorldModelProbe, :314-357 GRUEncoderOnly).

encoder -> Linear(E, 32) -> nn.GRU(32 + action_dim, deter_dim) -> probe, trained end to end through the probe loss
(probe_gradients=True) with ONE optimizer.  The encoder is whatever MultiEncoder builds for the section: the convolution stack on
64x64 frames, or - when models.dense_image_gate(conf) holds, the `minigrid` section - the DenseEncoder on a
categorical image.  As everywhere in this package the modules only own parameters; the step runs on the
C-ABI of libdreamer_hip.so: dm_conv_encoder_fwd(_planes), one dm_gemm_f32 for the squeeze (written straight into the leading 32
columns of the GRU's input rows), dm_gru_sequence_fwd (csrc/gru_seq.hip), the probe heads of models.py unchanged,
and in loss.backward() - on the caller's stream - the heads' backward WITH their input gradient, dm_gru_sequence_bwd, the squeeze
backward and dm_conv_encoder_bwd(_planes), all into the one flat gradient buffer of the optimizer.  The encoder is run by the methods
WorldModel runs it by - MultiEncoder.ingest / encode / backward - so on the dense branch the two encoder calls become
dm_dense_image_rows (from the float one-hot (T,B,C,S,S) or the integer class map (T,B,S,S): same bits), MLP.fwd, dm_elu_rows_fwd
into `embed`; backward dm_elu_rows_bwd in place on dembed, then dm_mlp_head_bwd without an input gradient.  No entry point is new.

Not built (NotImplementedError at construction): model in {vae, gru_vae, transformer_vae}; probe_gradients=False (the reference
then returns the Python float 0.0 as its first loss, which train.py:187 cannot backpropagate); probe_model='none';
vecobs_size > 0; amp=True; frames other than 64x64 outside the dense gate; image_encoder / image_decoder = 'dense' outside the
gate (the gate's own NotImplementedError).  Mid-sequence resets are not read, as in the reference (baselines.py:339: only reset[0] masks the
carried state).
"""
import ctypes
import math

import torch
import torch.nn as nn

from . import hip as H
from . import models as M
from .optim import FusedAdamW

SQUEEZE_DIM = 32          # baselines.py:321
OTHER_BASELINES = ('vae', 'gru_vae', 'transformer_vae')      # baselines.py:27-32


class GRUP(M._Params):
    """Parameter holder of torch.nn.GRU(input_size, hidden_size) (one layer): the names, shapes, order and default
    initialisation U(-1/sqrt(hidden), 1/sqrt(hidden)) of torch (init_weights_tf2 does not touch an nn.GRU, functions.py:81-94)."""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        self.weight_ih_l0 = nn.Parameter(torch.empty(3 * hidden_size, input_size))
        self.weight_hh_l0 = nn.Parameter(torch.empty(3 * hidden_size, hidden_size))
        self.bias_ih_l0 = nn.Parameter(torch.empty(3 * hidden_size))
        self.bias_hh_l0 = nn.Parameter(torch.empty(3 * hidden_size))
        k = 1.0 / math.sqrt(hidden_size)
        for p in self.parameters():
            nn.init.uniform_(p, -k, k)

    def ordered(self):
        return [self.weight_ih_l0, self.weight_hh_l0, self.bias_ih_l0, self.bias_hh_l0]


class GRUEncoderOnly(M._Params):
    """baselines.py:314-357."""

    def __init__(self, conf):
        super().__init__()
        self.state_dim = self.out_dim = conf.deter_dim
        self.encoder = M.MultiEncoder(conf)
        self.squeeze = M.LinearP(self.encoder.out_dim, SQUEEZE_DIM)
        self.rnn = GRUP(SQUEEZE_DIM + conf.action_dim, self.state_dim)

    def init_state(self, batch_size):
        return torch.zeros((1, batch_size, self.state_dim), device=next(self.rnn.parameters()).device)


class _GruProbeLoss(torch.autograd.Function):
    """loss_probe of the baseline: its gradient w.r.t. EVERY parameter of the model (probe heads, GRU, squeeze, encoder) is
    produced inside backward() on the caller's stream, into the `.grad` slots of the one optimizer when zero_grad() came first."""

    @staticmethod
    def forward(ctx, owner, pack, *params):
        ctx.owner, ctx.pack, ctx.params = owner, pack, params
        return pack['loss'].clone()

    @staticmethod
    def backward(ctx, grad_loss):
        owner, pk = ctx.owner, ctx.pack
        if pk.get('consumed'):
            raise RuntimeError('loss.backward() called twice (saved activations were released)')
        plist = list(ctx.params)
        flat, views, direct = M._flat_views(plist, grad_loss.device, getattr(owner, '_fused', None))
        owner._backward(pk, {id(p): v for p, v in zip(plist, views)})
        pk['consumed'] = True
        return (None, None) + M._finish_backward(owner, views, flat, direct, grad_loss)


class WorldModelProbe(nn.Module):
    """baselines.py:19-111 with conf.model='gru_probe'."""

    def __init__(self, conf):
        super().__init__()
        model = getattr(conf, 'model', 'dreamer')
        if model in OTHER_BASELINES:
            raise NotImplementedError(f'model={model!r}: of the baseline world models only gru_probe is built in the HIP path')
        if model != 'gru_probe':
            raise ValueError(model)                                       # baselines.py:36
        if conf.probe_model == 'none':
            raise NotImplementedError("model='gru_probe' with probe_model='none' has no loss to train on; pick map, goals or map+goals")
        if conf.probe_model not in ('map', 'goals', 'map+goals'):
            raise NotImplementedError(f'Unknown probe_model={conf.probe_model}')      # baselines.py:49
        if not conf.probe_gradients:
            raise NotImplementedError("model='gru_probe' needs probe_gradients=True: without it the reference's first loss is the "
                                      'Python float 0.0 (baselines.py:356), which the trainer cannot backpropagate')
        if getattr(conf, 'vecobs_size', 0):
            raise NotImplementedError("model='gru_probe' with vecobs_size > 0 is not built in the HIP path")
        if getattr(conf, 'amp', False):
            raise NotImplementedError("model='gru_probe' with amp=True is not built: the GRU sequence kernels are fp32")
        self.dense = M.dense_image_gate(conf)      # the DenseEncoder of the minigrid section; 'dense' outside the gate raises in it
        if not self.dense and conf.image_size != 64:
            raise NotImplementedError('the HIP convolution stack is built for 64x64 images')
        assert conf.action_dim > 0, 'Need to set action_dim to match environment'
        if conf.deter_dim % 4:
            raise NotImplementedError(f'deter_dim={conf.deter_dim}: the GRU sequence kernels need a multiple of 4')
        self.conf = conf
        self.probe_gradients = conf.probe_gradients
        self.wm = GRUEncoderOnly(conf)
        D_ = self.wm.out_dim
        if conf.probe_model == 'map':
            self.probe_model = M.MapProbeHead(D_ + 4, conf)
        elif conf.probe_model == 'goals':
            self.probe_model = M.GoalsProbe(D_, conf)
        else:
            self.probe_model = M.MapGoalsProbe(D_, conf)
        for m in self.modules():          # baselines.py:54-55: over ALL modules, the probe's Linears included
            M.init_weights_tf2(m)
        self._fused = None
        self._ws = None

    # ---- optimizer (baselines.py:57-76, the probe_gradients branch)
    def init_optimizers(self, lr, lr_actor=None, lr_critic=None, eps=1e-5):
        self._opt = FusedAdamW(list(self.parameters()), lr=lr, eps=eps)
        self._fused = self._opt
        return (self._opt,)

    def grad_clip(self, grad_clip, grad_clip_ac=None):
        if getattr(self, '_opt', None) is None:
            raise RuntimeError('call init_optimizers() before grad_clip(): clipping runs on the optimizer\'s flat buffer')
        mb = getattr(self, 'metric_buffer', None)
        if mb is not None and mb.device != self._opt.flat_grad.device:
            mb = None
        s = M.METRIC_SLOTS['grad_norm']
        return dict(grad_norm=self._opt.clip_grad_norm(grad_clip, None if mb is None else mb[s:s + 2]))

    def init_state(self, batch_size):
        return self.wm.init_state(batch_size)

    # ---- geometry / scratch
    def _shape(self, T, B):
        c = self.conf
        return H.make_shape(T=T, B=B, I=1, H=1, D=c.deter_dim, Hd=getattr(c, 'hidden_dim', 0), S=getattr(c, 'stoch_dim', 0),
                            C=getattr(c, 'stoch_discrete', 0), E=self.wm.encoder.out_dim, A=c.action_dim, mlp_hidden=M.MLP_HIDDEN,
                            # (dense: no convolution scratch in dm_workspace_bytes, as WorldModel.shape())
                            mlp_layers=4, cnn_depth=1 if self.dense else c.cnn_depth, img=c.image_size, img_ch=c.image_channels, flags=0)

    def _workspace(self, shp, T, B, device):
        In = SQUEEZE_DIM + self.conf.action_dim
        need = max(H.workspace_bytes(shp), int(H.lib().dm_gru_sequence_ws_bytes(T, B, In, self.conf.deter_dim)))
        if self.dense:      # the encoder MLP may be deeper than the four layers dm_workspace_bytes sizes the heads for
            deep = max(4, self.wm.encoder.encoder_image.hidden_layers)
            need = max(need, 4 * int(H.lib().dm_mlp_ws_floats(T * B, M.MLP_HIDDEN, deep)))
        self._ws = M._grow_ws(self._ws, need, device)
        return self._ws

    # ---- the step
    def training_step(self, obs, in_state, iwae_samples=1, imag_horizon=None, do_open_loop=False, do_image_pred=False,
                      do_dream_tensors=False):
        """Returns (losses, out_state, metrics, tensors, {}) with losses = (loss_probe,) (baselines.py:110: 0.0 + loss_probe),
        out_state (1, B, D) detached, metrics / tensors exactly the probe's.  imag_horizon and the three flags are accepted and
        have no effect, as in the reference.  obs: image (uint8 (T,B,64,64,C) or float (T,B,C,64,64); on the dense branch the float one-hot (T,B,C,S,S) or an
        integer class map (T,B,S,S), as WorldModel takes them), reset (T,B) - only
        reset[0] is read -, action_next (T,B,A), reward / terminal (T,B) with reward_input, and the probe's targets."""
        if iwae_samples != 1:
            raise AssertionError('iwae_samples must be 1 for the gru_probe baseline (baselines.py:335)')
        if 'action_next' not in obs:
            raise ValueError("model='gru_probe': obs['action_next'] is an input of the GRU (baselines.py:347)")
        for k in ('image', 'reset'):
            if k not in obs:
                raise ValueError(f"model='gru_probe': obs['{k}'] is required")
        c, wm = self.conf, self.wm
        image = obs['image']
        M._require_cuda(image, "obs['image']")
        T, B = obs['action_next'].shape[:2]
        N, dev = T * B, image.device
        D_, A_, E = c.deter_dim, c.action_dim, wm.encoder.out_dim
        In = SQUEEZE_DIM + A_
        train = torch.is_grad_enabled()
        shp = self._shape(T, B)
        h0 = in_state.float().contiguous()
        want = dict(action_next=(T, B, A_), reset=(T, B), in_state=(1, B, D_))
        got = dict(action_next=tuple(obs['action_next'].shape), reset=tuple(obs['reset'].shape), in_state=tuple(h0.shape))
        image, _, plane_r, plane_t, _ = wm.encoder.ingest(obs, T, B, shp, want, got)
        lib = H.lib()
        mbuf = torch.zeros(M.METRIC_BUF_FLOATS, device=dev)
        self.metric_buffer = mbuf
        ws = self._workspace(shp, T, B, dev)
        embed, enc_st = wm.encoder.encode(image, plane_r, plane_t, None, shp, ws)      # (in the caller's grad mode: it decides what is saved)
        with torch.no_grad():
            reset0 = obs['reset'][0].to(torch.uint8).contiguous()          # baselines.py:339-341: the batch start only
            # the GRU's input rows [squeeze(embed) | action_next] (baselines.py:346-348): the squeeze product writes the
            # leading 32 columns through its leading dimension
            x = torch.empty(N, In, device=dev)
            x[:, SQUEEZE_DIM:] = obs['action_next'].float().reshape(N, A_)
            H.call('dm_gemm_f32', 0, 0, N, SQUEEZE_DIM, E, H.fptr(embed), E, H.fptr(wm.squeeze.weight), E, H.fptr(x), In,
                   H.fptr(wm.squeeze.bias), None, 0, 0, H.ptr(ws), ws.numel(), H.stream())
            gru_p = H.gru_struct(*wm.rnn.ordered())
            gru_acts = torch.empty(int(lib.dm_gru_sequence_acts_floats(T, B, In, D_)), device=dev) if train else None
            Hs = torch.empty(N, D_, device=dev)
            H.call('dm_gru_sequence_fwd', T, B, In, D_, H.fptr(x), In, H.fptr(h0.view(B, D_)), H.ptr(reset0), ctypes.byref(gru_p),
                   H.fptr(gru_acts), H.fptr(Hs), D_, H.ptr(ws), ws.numel(), H.stream())
            out_state = Hs[(T - 1) * B:].clone().view(1, B, D_)
            features = Hs.view(T, B, 1, D_)

        # the probe (probes.py), on the features; in grad mode the heads hand back their backward packs
        pm = self.probe_model
        heads, metrics, tensors = [], {}, {}
        if isinstance(pm, M.MapGoalsProbe):
            parts = [pm.map_probe, pm.goals_probe]
        else:
            parts = [pm]
        loss = None
        for part in parts:
            r, m_, t_ = part.training_step(features, obs, mbuf=mbuf, _defer=True)
            metrics.update(**m_)
            tensors.update(**t_)
            if not train:
                l_ = r
            elif isinstance(part, M.MapProbeHead):
                l_, hp = r['loss'], [r]
            else:
                l_, hp = r
            if train:
                heads += hp
            with torch.no_grad():
                loss = l_ if loss is None else loss + l_
        if not train:
            return (loss,), out_state, metrics, tensors, {}
        pk = dict(loss=loss, heads=heads, T=T, B=B, shp=shp, x=x, gru_acts=gru_acts, Hs=Hs, ws=ws, **enc_st)
        self._last_pack = pk
        loss_probe = _GruProbeLoss.apply(self, pk, *self.parameters())
        return (loss_probe,), out_state, metrics, tensors, {}

    def _backward(self, pk, gof):
        """Probe heads (with their input gradient) -> dH -> GRU BPTT -> squeeze -> encoder; every gradient into gof[id(param)]."""
        c, wm = self.conf, self.wm
        T, B = pk['T'], pk['B']
        N, dev = T * B, pk['x'].device
        D_, A_, E = c.deter_dim, c.action_dim, wm.encoder.out_dim
        In = SQUEEZE_DIM + A_
        ws = pk['ws']
        # dH: the map head's input is [features | map_coord] (D + 4 wide) and comes first, so its dx OVERWRITES a buffer of that
        # width and the goals heads (input width D) accumulate into its leading D columns through the leading dimension
        ldd = max(hp['mlp'].in_dim for hp in pk['heads'])
        dH = torch.empty(N, ldd, device=dev)
        for i, hp in enumerate(pk['heads']):
            assert i == 0 or hp['mlp'].in_dim == D_
            hp['mlp'].bwd_into(gof, hp['x'], hp['ldx'], hp['rows'], hp['acts'], hp['dout'], hp['ws'], dx=dH, lddx=ldd, dx_accum=i > 0)
            for k in ('acts', 'dout', 'x'):
                hp.pop(k, None)
        rnn = wm.rnn
        gru_p = H.gru_struct(*rnn.ordered())
        gru_g = H.gru_struct(*[gof[id(p)] for p in rnn.ordered()])
        dx = torch.empty(N, In, device=dev)
        H.call('dm_gru_sequence_bwd', T, B, In, D_, H.fptr(pk['x']), In, ctypes.byref(gru_p), H.fptr(pk['gru_acts']), H.fptr(pk['Hs']),
               D_, H.fptr(dH), ldd, ctypes.byref(gru_g), H.fptr(dx), In, H.ptr(ws), ws.numel(), H.stream())
        # squeeze = Linear(E, 32): dW = dy^T embed, db = column sums of dy, dembed = dy W; dy = the leading 32 columns of dx
        sq = wm.squeeze
        H.call('dm_gemm_f32', 1, 1, SQUEEZE_DIM, E, N, H.fptr(dx), In, H.fptr(pk['embed']), E, H.fptr(gof[id(sq.weight)]), E,
               None, None, 0, 0, H.ptr(ws), ws.numel(), H.stream())
        H.call('dm_colsum', N, SQUEEZE_DIM, H.fptr(dx), In, H.fptr(gof[id(sq.bias)]), H.ptr(ws), ws.numel(), H.stream())
        dembed = torch.empty(N, E, device=dev)
        H.call('dm_gemm_f32', 0, 1, N, E, SQUEEZE_DIM, H.fptr(dx), In, H.fptr(sq.weight), E, H.fptr(dembed), E, None, None, 0, 0,
               H.ptr(ws), ws.numel(), H.stream())
        wm.encoder.backward(dembed, pk, gof, ws)
        for k in ('gru_acts', 'enc_acts', 'enc_x', 'embed', 'x', 'Hs'):
            pk.pop(k, None)
