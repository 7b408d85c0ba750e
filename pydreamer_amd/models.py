"""Dreamer / WorldModel / ActorCritic with pydreamer's module API, executing on hand-written HIP kernels.

Mirrors the reference module tree so `state_dict()` keys, shapes and optimizer grouping are identical
(reference: pydreamer/models/{dreamer,rssm,rnn,a2c,encoders,decoders,common,probes}.py), but no module here has a
torch `forward`: the nn.Modules own `nn.Parameter`s, and MultiEncoder / MultiDecoder and the decoder classes the methods that run
their kernels (each dense decoder's loss call is its own `loss`).  `Dreamer.training_step()` packs raw device pointers and
calls the C-ABI of libdreamer_hip.so (pydreamer_amd/hip.py) through three `torch.autograd.Function`s — world
model, actor, critic — so each of the 4 returned losses supports an independent `.backward()` exactly like the
reference (train.py:184-187).  There is no CPU path: tensors must live on a gfx950 device.

Supported configuration (everything else raises NotImplementedError): iwae_samples>=1 (also with the logging flags), gru_type in {gru, gru_layernorm,
gru_layernorm_dv2}, gru_layers 1..4, stoch_discrete>0 or 0 (Gaussian latents, also with iwae_samples>1), layer_norm True or False,
aux_critic, image_encoder/decoder='cnn' at 64x64 or both 'dense' on a categorical image of at most 16x16 cells (the `minigrid`
section; the gate is dense_image_gate(); obs['image'] is then the float one-hot (T,B,C,S,S) or the integer class map
(T,B,S,S) that ReplayFeed / DeviceReplay(image_categorical=C) hand over - same bits; the gru_probe baseline of baselines.py runs on
that path's DenseEncoder too), actor_dist in {onehot, tanh_normal, normal_tanh}, actor_grad='reinforce',
probe_model in {none, map, goals, map+goals} (map: the CatImageDecoder probe of the top-down map on the detached features, DESIGN
4.8; goals: two DenseNormalDecoders of the goal directions with the metrics of csrc/goals.hip, DESIGN 4.9, needs goals_size >= 1;
not with probe_gradients=True, whose gradient into the world model's features is not built), reward_input (cnn_depth in {8, 16, 32, 48, 64}: the reward and terminal planes are folded into the first
convolution), vecobs_size > 0 beside the image (an MLP encoder whose output sits behind the image embedding, a
DenseNormalDecoder with out_dim = vecobs_size), or vecobs_size > 0 with NO image at all - image_encoder and image_decoder both
empty (None or ''), the `vectorenv` section; the gate is imageless_gate(), DESIGN 4.12: the vecobs MLP's output is the RSSM's
embedding, the loss has no image term, obs needs no `image`, probe_model must be 'none', reward_input is ignored as in the
reference; everything in the RSSM, the heads and the actor-critic works as beside an image), reward_decoder_categorical = a list
of 2..32 reward values (DenseCategoricalSupportDecoder in place of the Normal reward head; it combines with all of
the above), critic_dist in {mse, twohot} (twohot: a categorical critic over critic_bins <= 256 symlog-spaced bins, read as a scalar
through ActorCritic.value) and return_norm in {none, percentile} (the actor's advantages over the running percentile range of the
imagined returns; not with a data-parallel group of more than one rank) - DESIGN 4.20; the task actor-critic only.  The world
model's share of the same, DESIGN 4.21: kl_free >= 0 (free bits per (t, b) row in nats: max(kl_free, KL) enters loss_model and a
row with KL <= kl_free sends no gradient into the posterior or the prior; loss_kl stays the exact KL, loss_kl_clip and kl_free_frac
are logged beside it; not with iwae_samples > 1) and reward_dist in {normal, twohot} (twohot: DenseTwoHotDecoder in place of the
Normal reward head - reward_twohot_bins <= 256 symlog-spaced bins over +-reward_twohot_range, two-hot cross-entropy against
symlog(reward), the mean decoded by symexp; not beside reward_decoder_categorical; it combines with all of the above).
"""
import contextlib
import ctypes
import math

import numpy as np
import torch
import torch.nn as nn

from . import hip as H
from .optim import FusedAdamW

MLP_HIDDEN = 400          # a2c.py:16, decoders.py:259,289
ACTOR_KINDS = {'onehot': 0, 'tanh_normal': 1, 'normal_tanh': 2}   # dm_shape.flags bits 0-1
REWARD_STD = 0.3989422804  # decoders.py:289
# -Normal(mu, std).log_prob(y) * std^2 = 0.5 (mu-y)^2 + NORMAL_LOSS_CONST per output (decoders.py:296-304), std = REWARD_STD
NORMAL_LOSS_CONST = REWARD_STD ** 2 * (math.log(REWARD_STD) + math.log(math.sqrt(2 * math.pi)))


# ---------------------------------------------------------------------------------------------------------------
# parameter holders (no forward): names/shapes follow torch.nn so state_dict keys equal the reference's
# ---------------------------------------------------------------------------------------------------------------
class _Params(nn.Module):
    def forward(self, *a, **k):
        raise RuntimeError('pydreamer_amd modules hold parameters only; compute runs in libdreamer_hip.so')


class LinearP(_Params):
    def __init__(self, in_dim, out_dim, bias=True):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_dim, in_dim))
        self.bias = nn.Parameter(torch.empty(out_dim)) if bias else None
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))           # torch.nn.Linear default (used by `ac`)
        if bias:
            bound = 1 / math.sqrt(in_dim)
            nn.init.uniform_(self.bias, -bound, bound)


class LayerNormP(_Params):
    def __init__(self, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.bias = nn.Parameter(torch.zeros(dim))


class ConvP(_Params):
    def __init__(self, shape, bias_dim):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(*shape))
        self.bias = nn.Parameter(torch.zeros(bias_dim))
        nn.init.xavier_uniform_(self.weight)


class GRUCellP(_Params):
    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.weight_ih = nn.Parameter(torch.empty(3 * hidden_size, input_size))
        self.weight_hh = nn.Parameter(torch.empty(3 * hidden_size, hidden_size))
        self.bias_ih = nn.Parameter(torch.zeros(3 * hidden_size))
        self.bias_hh = nn.Parameter(torch.zeros(3 * hidden_size))


class _Slot(_Params):
    """Parameter-free placeholder keeping nn.Sequential indices aligned with the reference (LN/ELU/Flatten slots)."""


def init_weights_tf2(m):
    """functions.py:81-94, applied to the world model only (dreamer.py:283-284)."""
    if isinstance(m, (LinearP, ConvP)):
        nn.init.xavier_uniform_(m.weight.data)
        if m.bias is not None:
            nn.init.zeros_(m.bias.data)
    if isinstance(m, GRUCellP):
        nn.init.xavier_uniform_(m.weight_ih.data)
        nn.init.orthogonal_(m.weight_hh.data)
        nn.init.zeros_(m.bias_ih.data)
        nn.init.zeros_(m.bias_hh.data)


class MLP(_Params):
    """common.py:37-65: model = Sequential[Linear, LayerNorm | NoNorm, ELU]*L + [Linear] (+Flatten if out_dim==1).
    layer_norm=False: the norm slots are parameter-free (common.py:68-74) and the library gets null LayerNorm pointers."""

    _base = 0          # Sequential index of the first Linear (DenseEncoder: 1, behind its nn.Flatten)

    def __init__(self, in_dim, out_dim, hidden_dim, hidden_layers, layer_norm=True):
        super().__init__()
        self.in_dim, self.out_dim, self.hidden_dim, self.hidden_layers = in_dim, out_dim, hidden_dim, hidden_layers
        self.layer_norm = bool(layer_norm)
        layers, dim = [_Slot()] * self._base, in_dim
        for _ in range(hidden_layers):
            layers += [LinearP(dim, hidden_dim), LayerNormP(hidden_dim) if layer_norm else _Slot(), _Slot()]
            dim = hidden_dim
        layers += [LinearP(dim, out_dim)]
        if out_dim == 1 or self._base:      # nn.Flatten of a scalar head; DenseEncoder's trailing activation()
            layers += [_Slot()]
        self.model = nn.Sequential(*layers)

    # --- C-ABI marshalling
    def tensors(self):
        L, o = self.hidden_layers, self._base
        w = [self.model[o + 3 * i].weight for i in range(L)] + [self.model[o + 3 * L].weight]
        b = [self.model[o + 3 * i].bias for i in range(L)] + [self.model[o + 3 * L].bias]
        g = [self.model[o + 3 * i + 1].weight for i in range(L)] if self.layer_norm else []
        be = [self.model[o + 3 * i + 1].bias for i in range(L)] if self.layer_norm else []
        return w, b, g, be

    def param_list(self):
        """Parameters in nn.Module.parameters() order (the order of the flat gradient buffer)."""
        return list(self.parameters())

    def struct(self):
        # precision: 1 = this head's contractions take bf16 operands (set by Dreamer from conf.amp; per call, no global)
        return H.mlp_struct(*self.tensors(), precision=getattr(self, 'precision', 0))

    def grad_struct(self, grads_by_param):
        w, b, g, be = self.tensors()
        pick = lambda ts: [grads_by_param[id(t)] for t in ts]
        return H.mlp_struct(pick(w), pick(b), pick(g), pick(be), cls=H.dm_mlp_grads)

    def acts_floats(self, rows):
        return int(H.lib().dm_mlp_acts_floats(rows, self.hidden_dim, self.hidden_layers))

    def fwd(self, x2d, ldx, rows, ws, acts=None, save_acts=True, sparse_cols=0, window=None, out=None):
        """x2d: device tensor whose rows (leading dim ldx floats) hold in_dim features. Returns (out, acts).
        save_acts=False (heads nobody differentiates: critic_target, the dream's reward / terminal heads, inference):
        no activation buffer is allocated or written; the library ping-pongs through the workspace.
        sparse_cols: the last sparse_cols input columns are mostly zero (the one-hot latent part of a feature row); same
        result for any input, cheaper first layer on large batches (dm_mlp_head_fwd_sparse).
        window=(rows_total, row0): x2d, `out` and `acts` are the FULL arrays of rows_total rows (given by the caller) and
        only rows [row0, row0 + rows) are computed (dm_mlp_head_fwd_rows); a row's result does not depend on the window."""
        need = 4 * int(H.lib().dm_mlp_ws_floats(rows, self.hidden_dim, self.hidden_layers))
        if ws.numel() < need:
            raise H.DreamerHipError(f'MLP.fwd: workspace of {ws.numel()} bytes, need {need} for {rows} rows')
        if window is not None:
            rows_total, row0 = window
            assert out is not None and out.shape[0] == rows_total and (acts is not None or not save_acts)
            st = self.struct()
            H.call('dm_mlp_head_fwd_rows', rows_total, row0, rows, self.in_dim, sparse_cols if 0 < sparse_cols < self.in_dim else 0,
                   self.hidden_dim, self.hidden_layers, self.out_dim, H.fptr(x2d), ldx, ctypes.byref(st),
                   H.fptr(acts) if save_acts else None, H.fptr(out), H.ptr(ws), ws.numel(), H.stream())
            return out, acts
        if acts is None and save_acts:
            acts = torch.empty(self.acts_floats(rows), device=x2d.device)
        out = torch.empty(rows, self.out_dim, device=x2d.device)
        st = self.struct()
        if 0 < sparse_cols < self.in_dim:
            H.call('dm_mlp_head_fwd_sparse', rows, self.in_dim, sparse_cols, self.hidden_dim, self.hidden_layers, self.out_dim,
                   H.fptr(x2d), ldx, ctypes.byref(st), H.fptr(acts), H.fptr(out), H.ptr(ws), ws.numel(), H.stream())
        else:
            H.call('dm_mlp_head_fwd', rows, self.in_dim, self.hidden_dim, self.hidden_layers, self.out_dim, H.fptr(x2d), ldx,
                   ctypes.byref(st), H.fptr(acts), H.fptr(out), H.ptr(ws), ws.numel(), H.stream())
        return out, acts

    def bwd(self, x2d, ldx, rows, acts, dout, ws, dx=None, lddx=0, dx_accum=False, scratch=False):
        """Returns (gradients in parameters() order, the flat buffer they are views of, direct): `direct` means the views
        ARE the optimizer's `.grad` slots (freshly zeroed), so autograd has nothing left to accumulate."""
        plist = self.param_list()
        flat, out, direct = _flat_views(plist, x2d.device, getattr(self, '_fused', None), scratch)
        self.bwd_into({id(p): v for p, v in zip(plist, out)}, x2d, ldx, rows, acts, dout, ws, dx, lddx, dx_accum)
        return out, flat, direct

    def bwd_into(self, gof, x2d, ldx, rows, acts, dout, ws, dx=None, lddx=0, dx_accum=False):
        """The backward pass with every parameter gradient written to gof[id(parameter)] (views of a caller's flat buffer that
        may hold other modules' gradients too).  dx: the input gradient (leading dim lddx), overwritten or, with dx_accum,
        added to; None: not computed."""
        st, gs = self.struct(), self.grad_struct(gof)
        H.call('dm_mlp_head_bwd', rows, self.in_dim, self.hidden_dim, self.hidden_layers, self.out_dim, H.fptr(x2d), ldx,
               ctypes.byref(st), H.fptr(acts), H.fptr(dout), ctypes.byref(gs), H.fptr(dx), lddx, 1 if dx_accum else 0, H.ptr(ws),
               ws.numel(), H.stream())


# ---------------------------------------------------------------------------------------------------------------
# world-model sub-modules (parameter trees only)
# ---------------------------------------------------------------------------------------------------------------
class ConvEncoder(_Params):
    """encoders.py:72-96."""

    def __init__(self, in_channels=3, cnn_depth=32):
        super().__init__()
        self.out_dim = cnn_depth * 32
        d = cnn_depth
        chans = [(in_channels, d), (d, 2 * d), (2 * d, 4 * d), (4 * d, 8 * d)]
        layers = []
        for ci, co in chans:
            layers += [ConvP((co, ci, 4, 4), co), _Slot()]
        layers += [_Slot()]
        self.model = nn.Sequential(*layers)

    def convs(self):
        return [self.model[i] for i in (0, 2, 4, 6)]


VECOBS_EMBED = 256        # encoders.py:34
DENSE_EMBED = 256         # encoders.py:25
DENSE_IMAGE_MAX_SIZE = 16


def dense_image_gate(conf):
    """True when conf selects the dense categorical image path, False for the convolution path.  The path is built
    for exactly one combination - every other use of 'dense' raises NotImplementedError naming what is outside:
    image_encoder == image_decoder == 'dense' on a categorical image (image_categorical) of at most 16 x 16 cells and at least 2
    classes, image_encoder_layers and image_decoder_layers in 1..DM_MAX_MLP_LAYERS - 1, no vecobs beside it, fp32 (amp off),
    image_decoder_min_prob in [0, 1); reward_input, layer_norm and the probe are free."""
    enc, dec = conf.image_encoder, conf.image_decoder
    if enc != 'dense' and dec != 'dense':
        return False
    top = H.DM_MAX_MLP_LAYERS - 1
    min_prob = float(getattr(conf, 'image_decoder_min_prob', 0) or 0)
    checks = [
        (enc == 'dense' and dec == 'dense', f'image_encoder={enc!r} with image_decoder={dec!r} (both must be dense)'),
        (bool(getattr(conf, 'image_categorical', False)), 'image_categorical is off (the decoder is a per-cell cross-entropy)'),
        (1 <= conf.image_size <= DENSE_IMAGE_MAX_SIZE, f'image_size={conf.image_size} (1..{DENSE_IMAGE_MAX_SIZE})'),
        (conf.image_channels >= 2, f'image_channels={conf.image_channels} (>= 2 classes)'),
        (1 <= conf.image_encoder_layers <= top, f'image_encoder_layers={conf.image_encoder_layers} (1..{top})'),
        (1 <= conf.image_decoder_layers <= top, f'image_decoder_layers={conf.image_decoder_layers} (1..{top})'),
        (not conf.vecobs_size, f'vecobs_size={conf.vecobs_size} (must be 0)'),
        (not getattr(conf, 'amp', False), 'amp=True (the dense image path is fp32)'),
        (0.0 <= min_prob < 1.0, f'image_decoder_min_prob={min_prob} (must lie in [0, 1))'),
    ]
    bad = [msg for ok, msg in checks if not ok]
    if bad:
        raise NotImplementedError("image_encoder / image_decoder = 'dense' is built for a categorical image only (both dense, "
                                  f'image_categorical, image_size <= {DENSE_IMAGE_MAX_SIZE}, image_channels >= 2, 1..{top} layers '
                                  'each, vecobs_size = 0, amp off, image_decoder_min_prob in [0, 1)); outside that gate: '
                                  + '; '.join(bad))
    return True


def _empty(x):
    return x is None or x == ''


def imageless_gate(conf):
    """True when conf selects a world model with no image at all (the `vectorenv` section): image_encoder and
    image_decoder BOTH empty (None or ''), vecobs_size >= 1.  Both empty without a vector observation is the reference's own
    assertion (encoders.py:38) -> ValueError; exactly one of the two empty stays NotImplementedError."""
    enc, dec = _empty(conf.image_encoder), _empty(conf.image_decoder)
    if not enc and not dec:
        return False
    if enc != dec:
        raise NotImplementedError(f'image_encoder={conf.image_encoder!r} with image_decoder={conf.image_decoder!r}: the image-less '
                                  'path needs both or neither of them empty (an encoder without its decoder, or the reverse, is '
                                  'not built in the HIP path)')
    if int(conf.vecobs_size or 0) < 1:
        raise ValueError('image_encoder and image_decoder are both empty and vecobs_size is 0: the encoder has no input at all '
                         '(the reference asserts `encoder_image or encoder_vecobs`, encoders.py:38)')
    return True


class DenseEncoder(MLP):
    """encoders.py:99-125: model = Sequential[Flatten, (Linear, LayerNorm | NoNorm, ELU) x L, Linear, ELU] - the Linears sit at
    1, 4, ..., 3L + 1, one behind the indices of `MLP`.  The marshalling, forward and backward are MLP's; the trailing ELU is
    dm_elu_rows_fwd / _bwd (MultiEncoder.dense_encode / MultiEncoder.backward)."""
    _base = 1

    def __init__(self, in_dim, hidden_layers, layer_norm=True):
        super().__init__(in_dim, DENSE_EMBED, MLP_HIDDEN, hidden_layers, layer_norm)


class CatImageDecoder(MLP):
    """decoders.py:183-254 with hidden_layers >= 1: model = Sequential[(Linear, LayerNorm | NoNorm, ELU) x L, Linear, Unflatten],
    the index layout of `MLP`; the loss and the decoded image are the kernels of csrc/cat_image.hip and dm_cat_image_loss_mix."""

    def __init__(self, in_dim, out_shape, hidden_layers, layer_norm=True, min_prob=0.0):
        C, S1, S2 = (int(x) for x in out_shape)
        super().__init__(in_dim, C * S1 * S2, MLP_HIDDEN, hidden_layers, layer_norm)
        self.out_shape, self.min_prob = (C, S1, S2), float(min_prob or 0)

    def target(self, image, NE):
        """The (NE, cells) class index of the image the loss is taken against (_cat_target_index)."""
        C, S1, S2 = self.out_shape
        return _cat_target_index(image, NE, C, S1 * S2)

    def loss(self, logits, target, N, loss, dlogits):
        """CatImageDecoder.loss (decoders.py:219-236) per row; min_prob = 0 is the map probe's kernel, bit for bit."""
        C, cells = self.out_shape[0], self.out_shape[1] * self.out_shape[2]
        if self.min_prob == 0:
            H.call('dm_cat_image_loss', N, 1, C, cells, H.fptr(logits), C * cells, H.ptr(target), H.fptr(loss), H.fptr(dlogits),
                   H.stream())
        else:
            H.call('dm_cat_image_loss_mix', N, 1, C, cells, H.fptr(logits), C * cells, H.ptr(target), self.min_prob, H.fptr(loss),
                   H.fptr(dlogits), H.stream())

    def logp(self, logits, target, NE):
        """The decoded image (decoders.py:247-251 with I = 1): per-cell normalised log-probabilities (NE, C, cells)."""
        C, cells = self.out_shape[0], self.out_shape[1] * self.out_shape[2]
        logp, acc = torch.empty(NE, C, cells, device=logits.device), torch.empty(NE, device=logits.device)
        H.call('dm_cat_image_pred', NE, 1, C, cells, H.fptr(logits), C * cells, H.ptr(target), None, H.fptr(logp), H.fptr(acc), None,
               H.stream())
        return logp


REWARD_INPUT_DEPTHS = (8, 16, 32, 48, 64)     # the depths of the direct layer-1 kernels (csrc/conv_direct.hip dm_enc_l1_direct_ok)


class MultiEncoder(_Params):
    """encoders.py:10-69 (image encoder, with or without the reward / terminal planes of reward_input; the vecobs MLP beside it,
    or alone on the image-less path).  Owns the parameters and runs the encoder for WorldModel and the gru_probe baseline:
    ingest() normalises what it reads of `obs`, encode() writes the (T*B, out_dim) embedding, backward() its gradients."""

    def __init__(self, conf):
        super().__init__()
        self.reward_input = bool(conf.reward_input)
        self.vecobs_size = int(conf.vecobs_size or 0)
        self.dense = dense_image_gate(conf)
        self.imageless = not self.dense and imageless_gate(conf)
        if not self.imageless:          # (image-less: image_size and image_channels are not read)
            self.image_channels, self.image_size = conf.image_channels, conf.image_size
        if self.dense:      # encoders.py:23-27: the flattened (C [+ 2], S, S) block through a DenseEncoder
            self.encoder_image = DenseEncoder(conf.image_size ** 2 * (conf.image_channels + (2 if self.reward_input else 0)),
                                              conf.image_encoder_layers, conf.layer_norm)
            self.encoder_vecobs = None
            self.out_dim = self.encoder_image.out_dim
            return
        if self.imageless:        # encoders.py:28-40,64-69: no image branch; reward_input is read inside it only, so it is ignored
            self.reward_input = False
            self.encoder_image = None
            self.encoder_vecobs = MLP(conf.vecobs_size, VECOBS_EMBED, MLP_HIDDEN, 2, conf.layer_norm)
            self.out_dim = VECOBS_EMBED
            return
        if conf.image_encoder != 'cnn':
            raise NotImplementedError("only image_encoder=cnn (with or without vecobs beside it) and the dense categorical image "
                                      'path (dense_image_gate) are built in the HIP path')
        if self.reward_input and (conf.cnn_depth not in REWARD_INPUT_DEPTHS or conf.image_channels != 3):
            raise NotImplementedError(f'reward_input is built for 3-channel frames and cnn_depth in {REWARD_INPUT_DEPTHS} '
                                      f'(got image_channels={conf.image_channels}, cnn_depth={conf.cnn_depth})')
        # encoders.py:15-18: + reward, terminal.  The two planes exist in the weight only: the kernels read the 3-channel frame
        self.encoder_image = ConvEncoder(in_channels=conf.image_channels + (2 if self.reward_input else 0), cnn_depth=conf.cnn_depth)
        # encoders.py:33-36,64-68: the vecobs embedding is concatenated behind the image embedding
        self.encoder_vecobs = MLP(conf.vecobs_size, VECOBS_EMBED, MLP_HIDDEN, 2, conf.layer_norm) if conf.vecobs_size else None
        self.out_dim = self.encoder_image.out_dim + (VECOBS_EMBED if conf.vecobs_size else 0)

    # ---- the step: ingest -> encode -> backward
    def ingest(self, obs, T, B, shp, want, got):
        """What the encoder reads of `obs`, normalised for the kernels: (image or None, u8, plane_r, plane_t, vecobs rows).
        want / got: the caller's own entries of the step's shape check; the encoder adds its entries and runs the check before it
        reshapes anything.  u8: the replay's native (T,B,H,W,C) uint8 frames are
        consumed AS THEY ARE - x/255-0.5 and HWC->CHW (preprocessing.py:21-29) happen inside the first conv's patch loader and
        inside the MSE kernel (dm_shape.flags bit DM_FLAG_IMAGE_U8, set on `shp` here); no float image is ever written (SURVEY
        8(f) N1).  Dense: the reference's float one-hot (T,B,C,S,S) (preprocessing.py:108-109) or an integer class map (T,B,S,S),
        same bits.  Image-less: no frame ingest, no obs['image']."""
        image, u8, NE = None, False, T * B
        if not self.imageless:
            image = obs['image']
            C, S = self.image_channels, self.image_size
            u8 = image.dtype == torch.uint8 and not self.dense
            want['image'] = (T, B, S, S, C) if u8 else (T, B, C, S, S)
            if self.dense:
                if not image.is_floating_point() and image.dim() == 5:
                    raise ValueError(f'the dense image path takes a float one-hot (T,B,C,S,S) image or an integer class map (T,B,S,S), '
                                     f'not a {image.dtype} frame of shape {tuple(image.shape)}')
                image = image.float().contiguous() if image.is_floating_point() else image.to(torch.int32).contiguous()
                if not image.is_floating_point():
                    want['image'] = (T, B, S, S)
            elif u8:
                if image.dim() != 5 or tuple(image.shape[2:]) != (S, S, C):
                    raise ValueError(f'uint8 image must be (T,B,{S},{S},{C}), got {tuple(image.shape)}')
                image = image.contiguous()
                shp.flags |= H.DM_FLAG_IMAGE_U8
            else:
                image = image.float().contiguous()
            got['image'] = tuple(image.shape)
        plane_r = plane_t = vecobs = None
        if self.reward_input:      # encoders.py:52-59: per-frame constants, (T,B) -> (NE,); never expanded to image planes
            for k in ('reward', 'terminal'):
                if k not in obs:
                    raise ValueError(f"reward_input: obs['{k}'] is an input of the encoder (encoders.py:52-59)")
                want[k], got[k] = (T, B), tuple(obs[k].shape)
        V = self.vecobs_size
        if V:
            if 'vecobs' not in obs:
                raise ValueError(f"vecobs_size={V}: obs['vecobs'] is an input of the encoder (encoders.py:64-66)")
            want['vecobs'], got['vecobs'] = (T, B, V), tuple(obs['vecobs'].shape)
        _check_shapes(want, got)
        if self.reward_input:
            plane_r = obs['reward'].float().contiguous().view(NE)
            plane_t = obs['terminal'].float().contiguous().view(NE)
        if V:
            vecobs = obs['vecobs'].float().contiguous().view(NE, V)
        return image, u8, plane_r, plane_t, vecobs

    def dense_encode(self, image, plane_r, plane_t, embed, NE, ws, save):
        """encoders.py:50-61,121-125: rows [image | reward plane | terminal plane] -> MLP -> ELU, written into `embed`.
        `image`: float one-hot (T,B,C,S,S), copied as it is, or an int32 class map (T,B,S,S).  Returns (rows, activations)."""
        enc = self.encoder_image
        onehot = image.is_floating_point()
        x = torch.empty(NE, enc.in_dim, device=embed.device)
        H.call('dm_dense_image_rows', NE, self.image_channels, self.image_size ** 2, H.fptr(image) if onehot else None,
               None if onehot else H.ptr(image), H.fptr(plane_r), H.fptr(plane_t), H.fptr(x), enc.in_dim, H.stream())
        pre, acts = enc.fwd(x, enc.in_dim, NE, ws, save_acts=save)
        H.call('dm_elu_rows_fwd', NE, enc.out_dim, H.fptr(pre), enc.out_dim, H.fptr(embed), embed.shape[1], H.stream())
        return x, acts

    def conv_structs(self, gof=None):
        """The convolution stack's parameters, or with gof their gradient slots, as the library takes them."""
        convs = self.encoder_image.convs()
        if gof is None:
            return H.conv_struct([m.weight for m in convs], [m.bias for m in convs])
        return H.conv_struct([gof[id(m.weight)] for m in convs], [gof[id(m.bias)] for m in convs], cls=H.dm_conv_grads)

    def encode(self, image, plane_r, plane_t, vecobs, shp_e, ws, forward_only=False):
        """The (T*B, E) embedding of the ingested observation and what backward() needs of this pass, under the pack's names:
        returns (embed, dict(image, plane_r, plane_t, vecobs, shp_e, embed, enc_x, enc_acts, ev_acts))."""
        NE, E = shp_e.T * shp_e.B, self.out_dim
        enc, V = self.encoder_image, self.vecobs_size
        enc_x = enc_acts = ev_acts = None
        if self.imageless:
            # encoders.py:64-69 with encoder_image = None: the vecobs MLP's (T*B, 256) output IS the RSSM's embed, no copy pass
            embed, ev_acts = self.encoder_vecobs.fwd(vecobs, V, NE, ws, save_acts=not forward_only and torch.is_grad_enabled())
        elif self.dense:
            embed = torch.empty(NE, E, device=image.device)
            enc_x, enc_acts = self.dense_encode(image, plane_r, plane_t, embed, NE, ws,
                                                save=not forward_only and torch.is_grad_enabled())
        else:
            enc_p = self.conv_structs()
            enc_acts = torch.empty(int(H.lib().dm_conv_encoder_acts_floats(ctypes.byref(shp_e))), device=image.device)
            embed = torch.empty(NE, E, device=image.device)
            if self.reward_input or V:
                # the image embedding is written as the leading E - 256 columns of the (NE, E) buffer (leading dimension E), the
                # vecobs embedding behind it: one buffer for the RSSM, no copy pass over the image embedding
                shp_c = H.dm_shape.from_buffer_copy(shp_e)
                shp_c.E = enc.out_dim                   # the convolution stack's own width
                H.call('dm_conv_encoder_fwd_planes', ctypes.byref(shp_c), H.ptr(image), ctypes.byref(enc_p), H.fptr(plane_r),
                       H.fptr(plane_t), H.fptr(enc_acts), H.fptr(embed), E, H.ptr(ws), ws.numel(), H.stream())
                if V:
                    ev, ev_acts = self.encoder_vecobs.fwd(vecobs, V, NE, ws, save_acts=not forward_only)
                    embed[:, enc.out_dim:].copy_(ev)
            else:
                H.call('dm_conv_encoder_fwd', ctypes.byref(shp_e), H.ptr(image), ctypes.byref(enc_p), H.fptr(enc_acts),
                       H.fptr(embed), H.ptr(ws), ws.numel(), H.stream())
        return embed, dict(image=image, plane_r=plane_r, plane_t=plane_t, vecobs=vecobs, shp_e=shp_e, embed=embed, enc_x=enc_x,
                           enc_acts=enc_acts, ev_acts=ev_acts)

    def backward(self, dembed, pk, gof, ws):
        """dembed (T*B, E) -> every encoder parameter's gradient into gof[id(parameter)]; pk: what encode() returned (or a pack
        that holds it).  dembed is consumed (the dense path's ELU derivative is applied in place).  No input gradient."""
        enc, ev, shp_e = self.encoder_image, self.encoder_vecobs, pk['shp_e']
        NE, E = shp_e.T * shp_e.B, self.out_dim
        if self.dense:      # through the trailing ELU (derivative from embed = ELU(pre), in place), then the MLP
            H.call('dm_elu_rows_bwd', NE, E, H.fptr(pk['embed']), E, H.fptr(dembed), E, H.fptr(dembed), E, H.stream())
            enc.bwd_into(gof, pk['enc_x'], enc.in_dim, NE, pk['enc_acts'], dembed, ws)
            return
        if self.imageless:      # the whole (T*B, 256) dembed is the vecobs MLP's output gradient
            ev.bwd_into(gof, pk['vecobs'], ev.in_dim, NE, pk['ev_acts'], dembed, ws)
            return
        enc_p, enc_g = self.conv_structs(), self.conv_structs(gof)
        if ev is not None:      # the vecobs encoder: its output gradient is the trailing 256 columns of dembed
            ev.bwd_into(gof, pk['vecobs'], ev.in_dim, NE, pk['ev_acts'], dembed[:, enc.out_dim:].contiguous(), ws)
        if self.reward_input or ev is not None:
            shp_c = H.dm_shape.from_buffer_copy(shp_e)
            shp_c.E = enc.out_dim
            H.call('dm_conv_encoder_bwd_planes', ctypes.byref(shp_c), H.ptr(pk['image']), ctypes.byref(enc_p),
                   H.fptr(pk['plane_r']), H.fptr(pk['plane_t']), H.fptr(pk['enc_acts']), H.fptr(dembed), E, ctypes.byref(enc_g),
                   H.ptr(ws), ws.numel(), H.stream())
        else:
            H.call('dm_conv_encoder_bwd', ctypes.byref(shp_e), H.ptr(pk['image']), ctypes.byref(enc_p),
                   H.fptr(pk['enc_acts']), H.fptr(dembed), ctypes.byref(enc_g), H.ptr(ws), ws.numel(), H.stream())


class ConvDecoder(_Params):
    """decoders.py:111-180 (mlp_layers=0)."""

    def __init__(self, in_dim, out_channels=3, cnn_depth=32):
        super().__init__()
        self.in_dim = in_dim
        d = cnn_depth
        self.model = nn.Sequential(
            LinearP(in_dim, d * 32), _Slot(),
            ConvP((d * 32, d * 4, 5, 5), d * 4), _Slot(),
            ConvP((d * 4, d * 2, 5, 5), d * 2), _Slot(),
            ConvP((d * 2, d, 6, 6), d), _Slot(),
            ConvP((d, out_channels, 6, 6), out_channels))

    def layers(self):
        return [self.model[i] for i in (0, 2, 4, 6, 8)]


def _reduce_i(x, NE, I, mode, iw=None):
    """TBI => TB (decoders.py:170-171,277-278,312-313) of x's NE * I rows -> (NE, ...).  mode 1: -logavgexp_i(-x) of a loss (`iw`
    (NE * I,) receives the importance weights softmax_i(-x)); mode 0: the mean over I of a prediction; mode 2: the sum."""
    out = x.new_empty(NE, *x.shape[1:])
    H.call('dm_reduce_i', NE, I, out.numel() // NE, H.fptr(x), mode, H.fptr(out), H.fptr(iw), H.stream())
    return out


class _DenseDecoder(_Params):
    """A dense decoder: `model` is the MLP, loss() the one kernel call behind its output `out` (N rows).
    loss(out, target, scale, grad, I, bins) -> (loss (N,), dout, mean, bin): dout = scale * d loss / d out, only with grad - the
    caller folds every factor of ITS loss into `scale`, none is computed here; `mean` the decoded mean per row; `bin` None but
    for the categorical head.  target=None is the mean-only form.
    buckets(target, bin) yields the (suffix, mask) pairs of the logprob_<name><suffix> splits (decoders.py:86-105)."""

    target_rows = True      # loss() takes one target per row (the (T,B) target expanded over I), not the (T,B) target itself


class DenseNormalDecoder(_DenseDecoder):
    """decoders.py:287-319.  nd: an Independent Normal over the out_dim outputs (dm_head_loss_normal_nd, at every width - the
    vecobs and goals heads) instead of the scalar head (dm_head_loss kind 0 - the reward head); the owner decides at
    construction."""

    def __init__(self, in_dim, hidden_layers, layer_norm=True, out_dim=1, nd=False):
        super().__init__()
        self.model = MLP(in_dim, out_dim, MLP_HIDDEN, hidden_layers, layer_norm)
        self.std = REWARD_STD
        self.nd = nd

    def loss(self, out, target=None, scale=0.0, grad=False, I=1, bins=False):
        (N, V), shape = out.shape, out.shape if self.nd else out.shape[:1]
        if target is None:      # the mean of a Normal is the MLP's output: nothing to launch
            return None, None, out.view(shape), None
        loss, dout, mean = out.new_empty(N), out.new_empty(shape) if grad else None, out.new_empty(shape)
        # (nd, decoders.py:295-304: the scalar head's std and constant per output)
        H.call(*(('dm_head_loss_normal_nd', N, V) if self.nd else ('dm_head_loss', 0, N)), H.fptr(out), H.fptr(target), scale,
               NORMAL_LOSS_CONST, H.fptr(loss), H.fptr(dout), H.fptr(mean), H.stream())
        return loss, dout, mean, None

    def buckets(self, target, bin):      # decoders.py:95-98: by the sign of the reward (the scalar head only)
        for sig in (() if self.nd else (-1, 1)):
            yield sig, torch.sign(target.float()) == sig


class DenseBernoulliDecoder(_DenseDecoder):
    """decoders.py:257-284."""

    def __init__(self, in_dim, hidden_layers, layer_norm=True):
        super().__init__()
        self.model = MLP(in_dim, 1, MLP_HIDDEN, hidden_layers, layer_norm)

    def loss(self, out, target=None, scale=0.0, grad=False, I=1, bins=False):
        N = out.shape[0]
        loss, dout, mean = (out.new_empty(N) if want else None for want in (target is not None, grad, True))
        H.call('dm_head_loss', 1, N, H.fptr(out), H.fptr(target), scale, 0.0, H.fptr(loss), H.fptr(dout), H.fptr(mean), H.stream())
        return loss, dout, mean, None

    def buckets(self, target, bin):      # decoders.py:101-105
        yield 1, target.float() > 0


CATSUP_MAX = 32           # dm_head_loss_catsup: at most 32 support values (a row group is at most half a wave)


def reward_support(conf):
    """The support of the categorical reward decoder, or None for the Normal head (decoders.py:34-41):
    clip_rewards_np(conf.reward_decoder_categorical, conf.clip_rewards) - the listed values are untransformed rewards, tanh /
    log1p is applied to the list (functions.py:153-160) - as float64, which the decoder rounds to fp32.  ValueError for fewer than
    two values or a non-finite one (log1p of a value <= -1: the reference would train on NaN); NotImplementedError for more than
    CATSUP_MAX values."""
    raw = conf.reward_decoder_categorical
    if raw is None or (isinstance(raw, (list, tuple)) and len(raw) == 0):
        return None
    if not isinstance(raw, (list, tuple)):
        raise ValueError(f'reward_decoder_categorical={raw!r}: a list of reward values is expected')
    x = np.asarray(raw, dtype=np.float64)
    if x.ndim != 1 or x.size < 2:
        raise ValueError(f'reward_decoder_categorical={raw!r}: at least 2 support values are needed')
    if x.size > CATSUP_MAX:
        raise NotImplementedError(f'reward_decoder_categorical with {x.size} support values: the HIP path is built for at most '
                                  f'{CATSUP_MAX} (dm_head_loss_catsup)')
    clip = conf.clip_rewards
    with np.errstate(all='ignore'):
        if clip == 'tanh':
            x = np.tanh(x)
        elif clip == 'log1p':
            x = np.log1p(x)
        elif clip:
            raise ValueError(f'clip_rewards={clip!r}')
    if not np.isfinite(x.astype(np.float32)).all():
        raise ValueError(f'reward_decoder_categorical={raw!r} with clip_rewards={clip!r} gives the support {x.tolist()}: every '
                         'support value must be finite')
    return x


class DenseCategoricalSupportDecoder(_DenseDecoder):
    """decoders.py:322-362: a categorical distribution over fixed support values.  `_support` is a frozen parameter as in the
    reference: it stands in state_dict() in front of model.model.* and in the world-model optimizer's parameter list, where it
    never receives a gradient.  Loss, decoded mean and the target's bin are dm_head_loss_catsup (csrc/cat_support.hip).
    Not built on the `meta` device: every other parameter of the model is re-initialised or loaded after to_empty(), but
    `_support` carries VALUES fixed at construction that no initialiser restores - a model materialised from `meta` would train
    against whatever the allocator left there.  Construct on a real device (CPU, then .to(device))."""

    def __init__(self, in_dim, support, hidden_layers, layer_norm=True):
        super().__init__()
        self.model = MLP(in_dim, len(support), MLP_HIDDEN, hidden_layers, layer_norm)
        self.support = np.array(support).astype(float)
        self._support = nn.Parameter(torch.tensor(self.support).to(torch.float), requires_grad=False)
        if self._support.is_meta:
            raise NotImplementedError('reward_decoder_categorical on the meta device is not built: `_support` holds values fixed '
                                      'at construction, which a meta tensor drops; construct the model on a real device')

    target_rows = False      # the target is the (T,B) reward itself: row r reads target r / I (decoders.py:340-362)

    def loss(self, out, target=None, scale=0.0, grad=False, I=1, bins=False):
        """`out`: (N, K) logits.  bins: `bin` (N / I,) int32, the support index of each target (not per IWAE sample)."""
        N, K = out.shape
        loss, dout, mean = (out.new_empty(shape) if want else None
                            for shape, want in ((N, target is not None), ((N, K), grad), (N, True)))
        bin = torch.empty(N // I, dtype=torch.int32, device=out.device) if bins else None
        H.call('dm_head_loss_catsup', N, I, K, H.fptr(out), K, H.fptr(self._support), H.fptr(target), scale, H.fptr(loss),
               H.fptr(dout), H.fptr(mean), H.ptr(bin), H.stream())
        return loss, dout, mean, bin

    def buckets(self, target, bin):      # decoders.py:86-94: one entry per support value; one nobody hit is 0 / 0 = NaN
        for i in range(self.model.out_dim):
            yield i, bin == i


REWARD_DISTS = ('normal', 'twohot')


def _check_twohot_support(bins, rng):
    if isinstance(bins, bool) or int(bins) != bins or not 2 <= bins <= 256:
        raise ValueError(f'reward_twohot_bins={bins}: 2 .. 256')
    if not (math.isfinite(rng) and rng > 0):
        raise ValueError(f'reward_twohot_range={rng}: a finite number > 0')


def reward_twohot_conf(conf):
    """(bins, range) of reward_dist='twohot', or None for the other reward heads.  ValueError for an unknown reward_dist, for
    'twohot' beside a non-empty reward_decoder_categorical, for reward_twohot_bins outside 2 .. 256 and for a
    reward_twohot_range that is not a finite number > 0 - the values are checked even while the head they belong to is off."""
    dist = getattr(conf, 'reward_dist', 'normal')
    bins, rng = getattr(conf, 'reward_twohot_bins', 255), getattr(conf, 'reward_twohot_range', 20.0)
    if dist not in REWARD_DISTS:
        raise ValueError(f'reward_dist={dist!r}: one of {REWARD_DISTS}')
    _check_twohot_support(bins, rng)
    if dist != 'twohot':
        return None
    raw = conf.reward_decoder_categorical
    if not (raw is None or (isinstance(raw, (list, tuple)) and len(raw) == 0)):
        raise ValueError(f"reward_dist='twohot' with reward_decoder_categorical={raw!r}: one reward head at a time")
    return int(bins), float(rng)


class DenseTwoHotDecoder(_DenseDecoder):
    """A symlog two-hot reward head (DreamerV3's; the reference has no counterpart): K logits over the bins
    linspace(-bin_range, bin_range, K) in symlog space, the two-hot cross-entropy against symlog(target) and the decoded mean
    symexp(sum_j softmax_j bins_j) - dm_twohot_head_loss (csrc/twohot.hip), the head form of the critic's dm_twohot_loss.  The loss
    is of order log K whatever the reward scale.  `bins` is a non-persistent buffer (a function of two config keys, as
    ActorCritic.bins): state_dict() holds the MLP alone, K wide at its output.  zero_output() - the owner calls it behind its
    weight initialisation - makes a fresh head predict reward 0 (equal logits over symmetric bins)."""

    target_rows = False      # row r reads target r / I (the kernel's own index, as the categorical head)

    def __init__(self, in_dim, bins=255, bin_range=20.0, hidden_layers=4, layer_norm=True):
        super().__init__()
        _check_twohot_support(bins, bin_range)
        self.K, self.bin_range = int(bins), float(bin_range)
        self.model = MLP(in_dim, self.K, MLP_HIDDEN, hidden_layers, layer_norm)
        self.register_buffer('bins', torch.linspace(-self.bin_range, self.bin_range, self.K), persistent=False)
        self.zero_output()

    def zero_output(self):
        out_layer = self.model.model[self.model._base + 3 * self.model.hidden_layers]
        nn.init.zeros_(out_layer.weight)
        nn.init.zeros_(out_layer.bias)

    def loss(self, out, target=None, scale=0.0, grad=False, I=1, bins=False):
        """`out`: (N, K) logits; target: the (N / I,) rewards themselves (untransformed; None: the mean-only form)."""
        N, K = out.shape
        loss, dout, mean = (out.new_empty(shape) if want else None
                            for shape, want in ((N, target is not None), ((N, K), grad), (N, True)))
        H.call('dm_twohot_head_loss', N, I, K, H.fptr(out), K, H.fptr(self.bins), H.fptr(target), scale, H.fptr(loss),
               H.fptr(dout), H.fptr(mean), H.stream())
        return loss, dout, mean, None

    def buckets(self, target, bin):      # by the sign of the reward, as the Normal head (decoders.py:95-98)
        for sig in (-1, 1):
            yield sig, torch.sign(target.float()) == sig


class MultiDecoder(_Params):
    """decoders.py:10-108.  Owns the heads' parameters and runs them for WorldModel and Dreamer: the image term (convolution,
    dense categorical or none) and the dense heads reward / terminal / vecobs - training forward (heads_loss), evaluation on
    prior-sample features (predict), the dream's windowed forward and mean decode (dream_buffers / dream_fwd / dream_means)."""

    def __init__(self, features_dim, conf):
        super().__init__()
        dense = self.dense = dense_image_gate(conf)
        imageless = self.imageless = not dense and imageless_gate(conf)
        self.features_dim = features_dim
        if conf.image_decoder != 'cnn' and not dense and not imageless:
            raise NotImplementedError(f'image_decoder={conf.image_decoder!r}: only image_decoder=cnn, the dense categorical image '
                                      'path (dense_image_gate) and the image-less path (imageless_gate) are built in the HIP path')
        support = reward_support(conf)
        twohot = reward_twohot_conf(conf)      # (checked before anything is allocated)
        self.image_weight, self.reward_weight, self.terminal_weight = conf.image_weight, conf.reward_weight, conf.terminal_weight
        if dense:      # decoders.py:23-28
            self.image = CatImageDecoder(features_dim, (conf.image_channels, conf.image_size, conf.image_size),
                                         conf.image_decoder_layers, conf.layer_norm, conf.image_decoder_min_prob)
        elif imageless:      # decoders.py:29-30: no image term in loss_reconstr, no image tensors
            self.image = None
        else:
            self.image = ConvDecoder(in_dim=features_dim, out_channels=conf.image_channels, cnn_depth=conf.cnn_depth)
        if not imageless:
            self.image_shape = (conf.image_channels, conf.image_size, conf.image_size)
        if support is not None:      # decoders.py:34-39
            self.reward = DenseCategoricalSupportDecoder(features_dim, support, conf.reward_decoder_layers, conf.layer_norm)
        elif twohot is not None:      # reward_dist='twohot' 
            self.reward = DenseTwoHotDecoder(features_dim, twohot[0], twohot[1], conf.reward_decoder_layers, conf.layer_norm)
        else:
            self.reward = DenseNormalDecoder(features_dim, conf.reward_decoder_layers, conf.layer_norm)
        self.reward_bins = 0 if support is None else len(support)      # the number of support values, 0 for the Normal head
        self.terminal = DenseBernoulliDecoder(features_dim, conf.terminal_decoder_layers, conf.layer_norm)
        self.vecobs_weight = conf.vecobs_weight
        if conf.vecobs_size:      # decoders.py:45-48
            self.vecobs = DenseNormalDecoder(features_dim, 4, conf.layer_norm, out_dim=conf.vecobs_size, nd=True)
        else:
            self.vecobs = None
        self.sparse_cols = conf.stoch_dim * conf.stoch_discrete      # the one-hot latent columns of a feature row (0: Gaussian)

    # ---- the dense heads: training forward (heads_loss), evaluation (predict), the dream (dream_buffers, dream_fwd, dream_means)
    def heads(self):
        """(name, decoder, weight in loss_model) in the order of the loss terms and of the backward's head list: reward and
        terminal, which every model has and whose schedules pair them ([:2]), then each further head ([2:])."""
        hs = [('reward', self.reward, self.reward_weight), ('terminal', self.terminal, self.terminal_weight)]
        return hs + [('vecobs', self.vecobs, self.vecobs_weight)] if self.vecobs is not None else hs

    @staticmethod
    def _targets(names, obs, pk):
        """name -> (the (T,B) target, its expansion over I: insert_dim, decoders.py:270,305); I = 1: the same tensor twice."""
        y = {n: pk['vecobs'] if n == 'vecobs' else obs[n].float().contiguous() for n in names}
        return {n: (t, t if pk['I'] == 1 else t.repeat_interleave(pk['I'], dim=int(n != 'vecobs')).contiguous()) for n, t in y.items()}

    def heads_loss(self, pk, obs, ws, gw):
        """Training forward of the dense heads on pk's T*B*I feature rows (decoders.py:57-83).  Returns name -> (loss (N,), rec (N,
        ...), target rows), per IWAE sample, and the backward's entries [(mlp, acts, dout)] in heads() order, dout = gw * weight /
        (T*B) * d loss / d out."""
        feat, NE, hs, res, bwd = pk['feat'], pk['T'] * pk['B'], self.heads(), {}, []
        N = feat.shape[0]
        for group in (hs[:2], hs[2:]):      # reward and terminal run side by side, each further head behind them
            y = self._targets([n for n, _, _ in group], obs, pk)
            outs = [head.model.fwd(feat, self.features_dim, N, ws, sparse_cols=self.sparse_cols) for _, head, _ in group]
            for (n, head, weight), (out, acts) in zip(group, outs):
                loss, dout, rec, _ = head.loss(out, y[n][head.target_rows], gw * weight / NE, grad=True, I=pk['I'])
                res[n] = (loss, rec, y[n][1])
                bwd.append((head.model, acts, dout))
        return res, bwd

    def predict(self, pk, feat, obs, ws):
        """The evaluation form (decoders.py:50-108 with extra_metrics), no gradients: every decoder on `feat`, pk's T*B*I rows with
        the latent part replaced (do_image_pred).  Returns (metrics, tensors): logprob_<name> and <name>_pred per decoder, reduced
        TBI => TB, and the NaN-masked splits logprob_<name><bucket> of each decoder's buckets() as (T,B) torch expressions."""
        T, B, I, shp = pk['T'], pk['B'], pk['I'], pk['shp']
        NE, N, F_ = T * B, T * B * I, self.features_dim
        tb = lambda x: x.view(T, B, *x.shape[1:])
        red = (lambda x, mode: x) if I == 1 else (lambda x, mode: _reduce_i(x, NE, I, mode))
        # loss and prediction (dense: normalised log-probabilities) of the image decoder; image-less: both None
        li, image_pred = self.decode(shp, feat, pk['image'], ws, target=pk.get('target'), loss=True)
        hs, lp, pred, bins = self.heads(), {}, {}, {}
        outs = [head.model.fwd(feat, F_, N, ws, save_acts=False)[0] for _, head, _ in hs[:2]]
        for n, head, _ in hs[2:]:
            y = self._targets([n], obs, pk)[n]
            l, _, p, _ = head.loss(head.model.fwd(feat, F_, N, ws, save_acts=False)[0], y[head.target_rows], I=I)
            lp[n], pred[n] = red(l, 1), red(p, 0)
        y = self._targets([n for n, _, _ in hs[:2]], obs, pk)
        per_sample = [head.loss(out, y[n][head.target_rows], I=I, bins=True) for (n, head, _), out in zip(hs[:2], outs)]
        if li is not None:
            lp['image'] = red(li, 1)
        for mode, into, k in ((1, lp, 0), (0, pred, 2)):      # -logavgexp over I for the losses, then the means of the predictions
            for (n, _, _), r in zip(hs[:2], per_sample):
                into[n], bins[n] = red(r[k], mode), r[3]
        if image_pred is not None:      # decoded.mean(dim=2), decoders.py:171
            image_pred = image_pred.view(NE, I, *image_pred.shape[1:])
            pred['image'] = image_pred.mean(1) if I > 1 else image_pred[:, 0]
        metrics, tensors = {}, {}
        for group in ([n for n in ('image', 'reward', 'terminal') if n in lp], *([n] for n, _, _ in hs[2:])):
            tensors.update({f'logprob_{n}': tb(lp[n]) for n in group})
            tensors.update({f'{n}_pred': tb(pred[n]) for n in group})
            metrics.update({f'logprob_{n}': lp[n].mean() for n in group})
        nan = torch.full((), float('nan'), device=feat.device)
        nanmean = lambda x: torch.nansum(x) / (~torch.isnan(x)).sum()     # functions.py:149-150
        for n, head, _ in hs:
            for s, mask in head.buckets(obs.get(n), bins.get(n)):
                x = torch.where(mask.view(T, B), tb(lp[n]), nan)
                metrics[f'logprob_{n}{s}'], tensors[f'logprob_{n}{s}'] = nanmean(x), x
        return metrics, tensors

    def dream_buffers(self, rows, device):
        """The reward and terminal heads' outputs over all `rows` imagined states, filled window by window (dream_fwd)."""
        return [torch.empty(rows, head.model.out_dim, device=device) for _, head, _ in self.heads()[:2]]

    def dream_fwd(self, feat, row0, n, ws, bufs):
        """Rows [row0, row0 + n) of the reward and terminal heads (dreamer.py:212-213); nobody differentiates them."""
        for (_, head, _), out in zip(self.heads()[:2], bufs):
            head.model.fwd(feat, self.features_dim, n, ws, save_acts=False, sparse_cols=self.sparse_cols, window=(out.shape[0], row0),
                           out=out)

    def dream_means(self, bufs):
        """(terminal, reward) means (rows,) behind the windows: only `.mean` of either distribution is read (dreamer.py:212-213)."""
        return self.terminal.loss(bufs[1])[2], self.reward.loss(bufs[0])[2]

    # ---- the image term: training forward (image_buffers, image_loss), backward (image_heads, image_bwd), evaluation (decode)
    def _conv_fwd(self, shp, feat, image, ws, acts, loss, pred):
        """ConvDecoder on shp's T*B*I feature rows: `loss` (rows,) = the MSE term against `image` and / or `pred` (rows, C, H, W),
        either may be None; `acts`: the activation buffer (dm_conv_decoder_acts_floats), which also keeps the NHWC prediction."""
        dl = self.image.layers()
        dec_p = H.conv_struct([m.weight for m in dl], [m.bias for m in dl])
        H.call('dm_conv_decoder_mse_fwd', ctypes.byref(shp), H.fptr(feat), self.features_dim, H.ptr(image), ctypes.byref(dec_p),
               H.fptr(acts), H.fptr(loss), H.fptr(pred), H.ptr(ws), ws.numel(), H.stream())

    def _conv_acts(self, shp, device):
        return torch.empty(int(H.lib().dm_conv_decoder_acts_floats(ctypes.byref(shp))), device=device)

    def image_buffers(self, shp, N, device):
        """(dec_acts, loss_image) of a training forward, either may be None.  Apart from image_loss() because they outlive the
        forward's tail: the caller allocates them on ITS stream, whichever stream the tail then runs on."""
        if self.imageless:
            return None, None
        return None if self.dense else self._conv_acts(shp, device), torch.empty(N, device=device)

    def image_loss(self, shp, feat, image, ws, acts, loss, gw):
        """Writes loss_image (one value per feature row) into `loss` and returns the pack entries of this pass: dec_acts, and on
        the dense path target, dec_logits and dlogits = d loss_model / d logits (gw: the data-parallel shard weight)."""
        if self.imageless:      # decoders.py:29-30: no image term
            return dict(dec_acts=None)
        if not self.dense:
            self._conv_fwd(shp, feat, image, ws, acts, loss, None)
            return dict(dec_acts=acts)
        # CatImageDecoder.training_step (decoders.py:238-254): MLP -> per-cell cross-entropy, I = 1
        dec, N, NE = self.image, feat.shape[0], shp.T * shp.B
        train = torch.is_grad_enabled()
        target = dec.target(image, NE)
        logits, acts = dec.fwd(feat, self.features_dim, N, ws, save_acts=train)
        dlogits = torch.empty_like(logits) if train else None
        dec.loss(logits, target, N, loss, dlogits)
        if train:      # d loss_model / d loss_image[r] = image_weight / (T*B), times the data-parallel shard weight
            scale = torch.full((1,), gw * self.image_weight / NE, device=feat.device)
            H.call('dm_scale_inplace', H.fptr(dlogits), dlogits.numel(), H.fptr(scale), H.stream())
        return dict(target=target, dec_acts=acts, dec_logits=logits, dlogits=dlogits)

    def image_heads(self, pk):
        """Dense path: the image decoder is one more dense head of the backward's head loop (its dx accumulates into dfeat)."""
        return [(self.image, pk['dec_acts'], pk['dlogits'])] if self.dense else []

    def image_bwd(self, pk, gof, dfeat, scale, iw, ws):
        """Convolution path: the MSE term's gradient (scale = d loss_model / d loss_image row, iw = the IWAE importance weights
        or None) through the decoder into gof and, accumulated, into dfeat."""
        if self.dense or self.imageless:
            return
        dl, F_ = self.image.layers(), self.features_dim
        dec_p = H.conv_struct([m.weight for m in dl], [m.bias for m in dl])
        dec_g = H.conv_struct([gof[id(m.weight)] for m in dl], [gof[id(m.bias)] for m in dl], cls=H.dm_conv_grads)
        H.call('dm_conv_decoder_mse_bwd_rows', ctypes.byref(pk['shp']), H.fptr(pk['feat']), F_, H.ptr(pk['image']), ctypes.byref(dec_p),
               H.fptr(pk['dec_acts']), scale, H.fptr(iw), ctypes.byref(dec_g), H.fptr(dfeat), F_, H.ptr(ws), ws.numel(), H.stream())

    def decode(self, shp, feat, image, ws, target=None, loss=False, raw=False):
        """Evaluation form, no gradients: decodes shp's T*B*I feature rows.  Returns (loss rows (N,) or None, prediction (N, C, H,
        W)); (None, None) without an image decoder.  `image` / `target`: what the loss is taken against (the convolution kernel
        takes the image argument also when no loss is asked for; the dense path's normalised log-probabilities need `target`).
        raw (dense only): the logits as they are (decoder.image.forward) instead of normalised log-probabilities."""
        if self.imageless:
            return None, None
        N, dev = feat.shape[0], feat.device
        li = torch.empty(N, device=dev) if loss else None
        if self.dense:
            logits, _ = self.image.fwd(feat, self.features_dim, N, ws, save_acts=False)
            if loss:
                self.image.loss(logits, target, N, li, None)
            pred = logits if raw else self.image.logp(logits, target, N)
        else:
            acts = self._conv_acts(shp, dev)
            pred = torch.empty(N, *self.image_shape, device=dev)
            self._conv_fwd(shp, feat, image, ws, acts, li, pred)
        return li, pred.view(N, *self.image_shape)

    def image_rec_thunk(self, pk):
        """image_rec (T,B,C,H,W) of a training forward, computed when somebody reads it (LazyTensors).  The thunk holds the
        decoder's logits / activations alive until the tensors dict is dropped."""
        T, B, I = pk['T'], pk['B'], pk['I']
        Cc, S, _ = self.image_shape
        if self.dense:
            def thunk(logits=pk['dec_logits'], target=pk['target']):
                with torch.no_grad():
                    return self.image.logp(logits, target, T * B).view(T, B, Cc, S, S)
            return thunk
        N, hw = T * B * I, S * S
        pred_off = int(H.lib().dm_conv_decoder_pred_offset(ctypes.byref(pk['shp'])))

        def thunk(acts=pk['dec_acts']):
            with torch.no_grad():
                pred = acts[pred_off:pred_off + N * hw * Cc].view(N, hw, Cc)                       # NHWC
                rec = pred.transpose(1, 2).contiguous().view(T, B, I, Cc, S, S)                    # -> (T,B,I,C,H,W)
                return rec[:, :, 0] if I == 1 else rec.mean(2)       # decoded.mean(dim=2), decoders.py:171 (logging only)
        return thunk


class NormGRUCellP(_Params):
    """rnn.py:95-104 (gru_layernorm): bias-free gate products, one LayerNorm(eps 1e-3) per gate."""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.weight_ih = LinearP(input_size, 3 * hidden_size, bias=False)
        self.weight_hh = LinearP(hidden_size, 3 * hidden_size, bias=False)
        self.ln_reset = LayerNormP(hidden_size)
        self.ln_update = LayerNormP(hidden_size)
        self.ln_newval = LayerNormP(hidden_size)


class NormGRUCellLateResetP(_Params):
    """rnn.py:117-125 (gru_layernorm_dv2): one LayerNorm over all three gates, update bias -1, late reset."""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.weight_ih = LinearP(input_size, 3 * hidden_size, bias=False)
        self.weight_hh = LinearP(hidden_size, 3 * hidden_size, bias=False)
        self.lnorm = LayerNormP(3 * hidden_size)


class GRUCellStack(_Params):
    """rnn.py:40-67; cell_type in {gru, gru_layernorm, gru_layernorm_dv2}, up to 4 layers of any of them: layer i owns
    columns [i*layer_size, (i+1)*layer_size) of the state."""

    def __init__(self, input_size, hidden_size, num_layers, cell_type):
        super().__init__()
        cells = dict(gru=GRUCellP, gru_layernorm=NormGRUCellP, gru_layernorm_dv2=NormGRUCellLateResetP)
        if cell_type not in cells or not 1 <= num_layers <= H.DM_MAX_GRU_LAYERS:
            raise NotImplementedError(f'gru_type={cell_type!r}, gru_layers={num_layers} not built in the HIP path')
        layer_size = hidden_size // num_layers
        assert layer_size * num_layers == hidden_size, 'Must be divisible'
        if layer_size % 4:
            raise NotImplementedError(f'deter_dim / gru_layers = {layer_size} must be a multiple of 4 in the HIP path')
        self.cell_type, self.num_layers = cell_type, num_layers
        self.layers = nn.ModuleList([cells[cell_type](input_size, layer_size)] +
                                    [cells[cell_type](layer_size, layer_size) for _ in range(num_layers - 1)])


class RSSMCell(_Params):
    """rssm.py:97-203."""

    def __init__(self, embed_dim, action_dim, deter_dim, stoch_dim, stoch_discrete, hidden_dim, gru_layers, gru_type, layer_norm):
        super().__init__()
        norm = LayerNormP if layer_norm else (lambda n: _Slot())       # NoNorm (common.py:68-74): no parameters
        self.stoch_dim, self.stoch_discrete, self.deter_dim = stoch_dim, stoch_discrete, deter_dim
        # discrete latents: stoch_dim one-hot groups of stoch_discrete; Gaussian latents (stoch_discrete = 0): z is stoch_dim
        # wide and the prior / posterior heads emit (mean | raw std)                                 (rssm.py:103,112,117)
        Z, ZP = stoch_dim * (stoch_discrete or 1), stoch_dim * (stoch_discrete or 2)
        self.z_mlp = LinearP(Z, hidden_dim)
        self.a_mlp = LinearP(action_dim, hidden_dim, bias=False)
        self.in_norm = norm(hidden_dim)
        self.gru = GRUCellStack(hidden_dim, deter_dim, gru_layers, gru_type)
        self.prior_mlp_h = LinearP(deter_dim, hidden_dim)
        self.prior_norm = norm(hidden_dim)
        self.prior_mlp = LinearP(hidden_dim, ZP)
        self.post_mlp_h = LinearP(deter_dim, hidden_dim)
        self.post_mlp_e = LinearP(embed_dim, hidden_dim, bias=False)
        self.post_norm = norm(hidden_dim)
        self.post_mlp = LinearP(hidden_dim, ZP)

    def ordered(self):
        """Tensors in the DM_RSSM_* order of include/dreamer_hip.h (None for slots this cell type does not have)."""
        named = dict(self.named_parameters())
        return [named.get(n) for n in H.rssm_param_names(self.gru.cell_type, self.gru.num_layers)]      # None: slot not present

    def init_state(self, batch_size):
        dev = self.z_mlp.weight.device
        return (torch.zeros((batch_size, self.deter_dim), device=dev),
                torch.zeros((batch_size, self.stoch_dim * (self.stoch_discrete or 1)), device=dev))


class RSSMCore(_Params):
    """rssm.py:15-93."""

    def __init__(self, embed_dim, action_dim, deter_dim, stoch_dim, stoch_discrete, hidden_dim, gru_layers, gru_type, layer_norm):
        super().__init__()
        self.cell = RSSMCell(embed_dim, action_dim, deter_dim, stoch_dim, stoch_discrete, hidden_dim, gru_layers, gru_type, layer_norm)

    def init_state(self, batch_size):
        return self.cell.init_state(batch_size)


class NoProbeHead(nn.Module):
    """probes.py:140-150: keeps the 4-loss / 4-optimizer structure."""

    def __init__(self):
        super().__init__()
        self.dummy = nn.Parameter(torch.zeros(1), requires_grad=True)

    def training_step(self, features, obs):
        return torch.square(self.dummy), {}, {}


class MapProbeHead(_Params):
    """probes.py:32-86 with the dense CatImageDecoder (decoders.py:183-254): an MLP from [features | map_coord] to the
    (map_channels, map_size, map_size) logits of the top-down map, trained by a per-cell cross-entropy on the DETACHED features -
    the reference's memory evaluation for maze environments.  `self.decoder` is the MLP holder, so the keys are
    probe_model.decoder.model.{0,1,3,4,...}.{weight,bias} as the reference's Sequential names them; torch's default Linear
    init (init_weights_tf2 is applied to the world model only, dreamer.py:283).  The loss, its gradient, the decoded map and the
    accuracies are the kernels of csrc/cat_image.hip; all of them fp32 (conf.amp reaches the MLP's products only).
    The gradient INTO the features (probe_gradients=True) is not built: Dreamer() refuses that combination."""

    def __init__(self, map_state_dim, conf):
        super().__init__()
        if getattr(conf, 'map_decoder', 'dense') != 'dense':
            raise NotImplementedError(conf.map_decoder)                    # probes.py:43
        self.map_channels, self.map_size = int(getattr(conf, 'map_channels', 0)), int(getattr(conf, 'map_size', 0))
        if self.map_channels < 1 or self.map_size < 1:
            raise ValueError(f"probe_model='map' needs map_size >= 1 and map_channels >= 1 (got map_size={self.map_size}, "
                             f'map_channels={self.map_channels})')
        layers = int(getattr(conf, 'map_hidden_layers', 4))
        if layers < 1:
            raise NotImplementedError('map_hidden_layers=0 (a single Linear, decoders.py:205-209) is not built in the HIP path')
        self.decoder = MLP(map_state_dim, self.map_channels * self.map_size ** 2, int(getattr(conf, 'map_hidden_dim', 1024)), layers,
                           conf.layer_norm)
        self._ws = None

    def _workspace(self, rows, device):
        d = self.decoder
        need = 4 * int(H.lib().dm_mlp_ws_floats(rows, d.hidden_dim, d.hidden_layers))
        self._ws = _grow_ws(self._ws, need, device)
        return self._ws

    def training_step(self, features, obs, mbuf=None, _defer=False):
        """features (T,B,I,F), detached.  Returns (loss_probe, metrics, tensors) with the reference's names: metrics loss_map,
        acc_map, acc_map_seen (only with obs['map_seen_mask']); tensors map_rec (T,B,C,H,W), loss_map (T,B), acc_map (T,B).
        _defer (MapGoalsProbe): in grad mode the first result is the head's backward pack instead of an autograd loss."""
        _require_cuda(features, 'features')
        T, B, I, F_ = features.shape
        C, S = self.map_channels, self.map_size
        cells, N, NE, dev = S * S, T * B * I, T * B, features.device
        for k in ('map', 'map_coord'):
            if k not in obs:
                raise ValueError(f"probe_model='map': obs['{k}'] is an input of the map probe (probes.py:54-57)")
        m = obs['map']
        onehot = m.is_floating_point()
        want = dict(map=(T, B, C, S, S) if onehot else (T, B, S, S), map_coord=(T, B, 4))
        got = dict(map=tuple(m.shape), map_coord=tuple(obs['map_coord'].shape))
        seen = obs.get('map_seen_mask')
        if seen is not None:
            want['map_seen_mask'], got['map_seen_mask'] = (T, B, S, S), tuple(seen.shape)
        _check_shapes(want, got)
        train = torch.is_grad_enabled()
        with torch.no_grad():
            # target.argmax(dim=-3) (decoders.py:221); an integer class map is taken as it is
            target = _cat_target_index(m, NE, C, cells)
            # torch.cat((features, insert_dim(map_coord, 2, I)), -1) (probes.py:54-55)
            feat2d = features.reshape(N, F_)
            x = torch.empty(N, F_ + 4, device=dev)
            H.call('dm_cat_concat_rows', N, I, F_, 4, H.fptr(feat2d.contiguous()), F_, H.fptr(obs['map_coord'].float().contiguous()),
                   H.fptr(x), H.stream())
            ws = self._workspace(N, dev)
            dec = self.decoder
            logits, acts = dec.fwd(x, F_ + 4, N, ws, save_acts=train)
            ld = C * cells
            loss_tbi = torch.empty(N, device=dev)
            dlogits = torch.empty(N, ld, device=dev) if train else None
            H.call('dm_cat_image_loss', N, I, C, cells, H.fptr(logits), ld, H.ptr(target), H.fptr(loss_tbi), H.fptr(dlogits), H.stream())
            gw = float(getattr(self, 'grad_weight', 1.0))          # data-parallel shard weight B_r/B (dist.attach), gradients only
            if I == 1:
                loss_tb = loss_tbi
                if train:      # d loss_probe / d loss_tb = 1 / (T*B)
                    H.call('dm_scale_inplace', H.fptr(dlogits), N * ld, H.fptr(torch.full((1,), gw / NE, device=dev)), H.stream())
            else:              # loss_tb = -logavgexp_i(-loss_tbi) (decoders.py:245); its importance weights scale the row gradients
                iw = torch.empty(N, device=dev)
                loss_tb = _reduce_i(loss_tbi, NE, I, 1, iw=iw)
                if train:
                    H.call('dm_scale_rows', N, ld, H.fptr(dlogits), ld, H.fptr(iw), gw / NE, H.stream())
            map_rec = torch.empty(T, B, C, S, S, device=dev)
            acc = torch.empty(NE, device=dev)
            acc_seen = seen_i = None
            if seen is not None:
                seen_i, acc_seen = seen.to(torch.int32).contiguous(), torch.empty(NE, device=dev)
            H.call('dm_cat_image_pred', NE, I, C, cells, H.fptr(logits), ld, H.ptr(target), H.ptr(seen_i), H.fptr(map_rec), H.fptr(acc),
                   H.fptr(acc_seen), H.stream())
            if mbuf is None:
                mbuf = torch.zeros(METRIC_BUF_FLOATS, device=dev)
            s0 = METRIC_SLOTS['loss_map']
            _multi_sum([(loss_tb, 1.0 / NE), (acc, 1.0 / NE)], dev, out=mbuf[s0:s0 + 2])      # acc_map has no NaN: nanmean = mean
            metrics = dict(loss_map=mbuf[s0], acc_map=mbuf[s0 + 1])
            if acc_seen is not None:      # nanmean (functions.py:149-150): frames without a seen cell are NaN and do not count
                mbuf[s0 + 2].copy_(torch.nansum(acc_seen) / (~torch.isnan(acc_seen)).sum())
                metrics['acc_map_seen'] = mbuf[s0 + 2]
            tensors = dict(map_rec=map_rec, loss_map=loss_tb.view(T, B), acc_map=acc.view(T, B))
        if not train:
            return mbuf[s0].clone(), metrics, tensors
        pk = dict(mlp=dec, loss=mbuf[s0], x=x, ldx=F_ + 4, rows=N, acts=acts, dout=dlogits, ws=ws)
        self._last_pack = pk
        if _defer:
            return pk, metrics, tensors
        return _ProbeLoss.apply(self, dict(loss=mbuf[s0], heads=[pk]), *dec.param_list()), metrics, tensors


GOAL_KEYS = ('goal_direction', 'goals_direction')      # probes.py:93-96, the ModuleDict's order


class _Decoders(_Params):
    """The nn.ModuleDict of probes.py:93: a parameter-only holder whose children keep their insertion order."""


class GoalsProbe(_Params):
    """probes.py:89-137: two DenseNormalDecoders on the DETACHED, bare features (no map_coord behind them) - `goal_direction`
    (out_dim 2) and `goals_direction` (out_dim 2 * goals_size), each with hidden_layers=4 and layer_norm=True whatever
    conf.layer_norm says (probes.py:94-95).  Keys probe_model.decoders.{goal_direction,goals_direction}.model.model.{0,1,3,...};
    torch's default Linear init, as for the map probe.  Forward and backward of the heads are MLP.fwd / dm_mlp_head_bwd, the
    Normal loss DenseNormalDecoder.loss (nd), the IWAE reduction _reduce_i / dm_scale_rows; mse_goals, var_goals and the six
    mse_goal_age* come from one dm_goals_stats call (csrc/goals.hip) that writes them into the step's metric buffer."""

    def __init__(self, state_dim, conf):
        super().__init__()
        self.goals_size = int(getattr(conf, 'goals_size', 0))
        if self.goals_size < 1:      # the reference would build a zero-width decoder
            raise NotImplementedError(f"probe_model={getattr(conf, 'probe_model', 'goals')!r} needs goals_size >= 1 "
                                      f'(got goals_size={self.goals_size}): a zero-width goals decoder is not built in the HIP path')
        self.decoders = _Decoders()
        self.decoders.add_module('goal_direction', DenseNormalDecoder(state_dim, 4, True, out_dim=2, nd=True))
        self.decoders.add_module('goals_direction', DenseNormalDecoder(state_dim, 4, True, out_dim=2 * self.goals_size, nd=True))
        self._ws = None

    def heads(self):
        return [getattr(self.decoders, k).model for k in GOAL_KEYS]

    def _workspace(self, rows, device):
        need = 4 * int(H.lib().dm_mlp_ws_floats(rows, MLP_HIDDEN, 4))
        self._ws = _grow_ws(self._ws, need, device)
        return self._ws

    def training_step(self, features, obs, mbuf=None, _defer=False):
        """features (T,B,I,F), detached.  Returns (loss_probe, metrics, tensors) with the reference's names: metrics
        loss_goal_direction, loss_goals_direction, mse_goals, var_goals and, with obs['goals_visage'], mse_goal_age{0,5,10,50,200,
        1000}; tensors loss_<key> (T,B) and <key>_pred (T,B,out_dim).  _defer (MapGoalsProbe): in grad mode the first result is
        (loss, backward packs) instead of an autograd loss."""
        _require_cuda(features, 'features')
        T, B, I, F_ = features.shape
        G = self.goals_size
        N, NE, dev = T * B * I, T * B, features.device
        for k in GOAL_KEYS:
            if k not in obs:
                raise ValueError(f"probe_model='goals': obs['{k}'] is a target of the goals probe (probes.py:102-105)")
        want = dict(goal_direction=(T, B, 2), goals_direction=(T, B, 2 * G))
        got = {k: tuple(obs[k].shape) for k in GOAL_KEYS}
        visage = obs.get('goals_visage')
        if visage is not None:
            want['goals_visage'], got['goals_visage'] = (T, B, G), tuple(visage.shape)
        _check_shapes(want, got)
        train = torch.is_grad_enabled()
        with torch.no_grad():
            feat2d = features.reshape(N, F_).contiguous()
            ws = self._workspace(N, dev)
            gw = float(getattr(self, 'grad_weight', 1.0))          # data-parallel shard weight B_r/B (dist.attach), gradients only
            if mbuf is None:
                mbuf = torch.zeros(METRIC_BUF_FLOATS, device=dev)
            s0 = GOALS_METRIC_SLOTS['loss_goal_direction']
            packs, metrics, tensors, means, targets = [], {}, {}, [], {}
            for n, (key, head) in enumerate(self.decoders.named_children()):      # GOAL_KEYS, in that order
                mlp, V = head.model, head.model.out_dim
                target = targets[key] = obs[key].float().contiguous().view(NE, V)
                rows_t = target.repeat_interleave(I, dim=0).contiguous() if I > 1 else target      # insert_dim(target, 2, I), decoders.py:309
                mu, acts = mlp.fwd(feat2d, F_, N, ws, save_acts=train)
                # d loss_probe / d loss_tb = 1 / (T*B); with I > 1 the importance weights come in below
                loss_tb, dmu, pred, _ = head.loss(mu, rows_t, gw / NE if I == 1 else 1.0, grad=train)
                if I > 1:          # loss_tb = -logavgexp_i(-loss_tbi), decoded.mean.mean(dim=2) (decoders.py:313-314)
                    iw = torch.empty(N, device=dev)
                    loss_tb, pred = _reduce_i(loss_tb, NE, I, 1, iw=iw), _reduce_i(pred, NE, I, 0)
                    if train:
                        H.call('dm_scale_rows', N, V, H.fptr(dmu), V, H.fptr(iw), gw / NE, H.stream())
                means.append((loss_tb, 1.0 / NE))
                metrics[f'loss_{key}'] = mbuf[s0 + n]
                tensors[f'loss_{key}'] = loss_tb.view(T, B)
                tensors[f'{key}_pred'] = pred.view(T, B, V)
                if train:
                    packs.append(dict(mlp=mlp, x=feat2d, ldx=F_, rows=N, acts=acts, dout=dmu, ws=ws))
            _multi_sum(means, dev, out=mbuf[s0:s0 + 2])
            loss = mbuf[s0] + mbuf[s0 + 1]          # loss_total = sum over the keys of loss.mean() (probes.py:106)
            # mse_goals, var_goals and the age buckets (probes.py:113-135): one call, straight into the metric slots
            s1 = GOALS_METRIC_SLOTS['mse_goals']
            vis = None if visage is None else visage.float().contiguous()
            gws = torch.empty(max(1, int(H.lib().dm_goals_stats_ws_floats(NE, G))), device=dev)
            H.call('dm_goals_stats', NE, G, H.fptr(targets['goals_direction']), H.fptr(tensors['goals_direction_pred'].contiguous()),
                   H.fptr(vis), ctypes.c_void_p(mbuf.data_ptr() + 4 * s1), H.fptr(gws), gws.numel() * 4, H.stream())
            names = GOALS_STAT_NAMES if vis is not None else GOALS_STAT_NAMES[:2]
            metrics.update({k: mbuf[GOALS_METRIC_SLOTS[k]] for k in names})
        if not train:
            return loss, metrics, tensors
        self._last_packs = packs
        if _defer:
            return (loss, packs), metrics, tensors
        return _ProbeLoss.apply(self, dict(loss=loss, heads=packs), *self.parameters()), metrics, tensors


class MapGoalsProbe(_Params):
    """probes.py:15-29: the map probe on [features | map_coord] and the goals probe on the bare features; the loss is the sum of
    both, metrics and tensors are the union.  Keys probe_model.map_probe.decoder.* then probe_model.goals_probe.decoders.*.
    One autograd node and ONE claim of the probe optimizer's gradient buffer serve the three MLPs (_ProbeLoss)."""

    def __init__(self, state_dim, conf):
        super().__init__()
        self.map_probe = MapProbeHead(state_dim + 4, conf)
        self.goals_probe = GoalsProbe(state_dim, conf)

    @property
    def grad_weight(self):
        return getattr(self.map_probe, 'grad_weight', 1.0)

    @grad_weight.setter
    def grad_weight(self, w):
        self.map_probe.grad_weight = self.goals_probe.grad_weight = w

    def training_step(self, features, obs, mbuf=None):
        if mbuf is None:
            mbuf = torch.zeros(METRIC_BUF_FLOATS, device=features.device)
        r_map, metrics_map, tensors_map = self.map_probe.training_step(features, obs, mbuf=mbuf, _defer=True)
        r_goals, metrics_goals, tensors_goals = self.goals_probe.training_step(features, obs, mbuf=mbuf, _defer=True)
        metrics, tensors = dict(**metrics_map, **metrics_goals), dict(**tensors_map, **tensors_goals)
        if not torch.is_grad_enabled():
            return r_map + r_goals, metrics, tensors
        loss_goals, packs = r_goals
        with torch.no_grad():
            loss = r_map['loss'] + loss_goals
        return _ProbeLoss.apply(self, dict(loss=loss, heads=[r_map] + packs), *self.parameters()), metrics, tensors


def _torch_actor_distribution(actor_dist, y):
    """The distribution object Dreamer.inference hands to the acting process (a2c.py:43-55, functions.py:59-78); the
    parameters come from the HIP actor, the torch.distributions wrapper is only the return type of the reference API."""
    import torch.distributions as D
    import torch.nn.functional as F
    if actor_dist == 'onehot':
        return D.OneHotCategorical(logits=y)
    mean_, std_ = y.chunk(2, -1)
    if actor_dist == 'normal_tanh':
        return D.Independent(D.Normal(torch.tanh(mean_), torch.sigmoid(std_) + 0.01), 1)
    normal = D.Independent(D.Normal(5 * torch.tanh(mean_ / 5), F.softplus(std_) + 0.1), 1)
    dist = D.TransformedDistribution(normal, [D.TanhTransform()])
    dist.entropy = normal.entropy
    return dist


class _Mean:
    """Stand-in for the torch.distributions objects Dreamer.dream returns: only `.mean` is consumed (dreamer.py:155-156)."""

    def __init__(self, mean):
        self.mean = mean


# ---------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------
def _flat_views(plist, device, fused=None, scratch=False):
    """Gradient buffers for one backward pass: (flat, per-parameter views, direct).
    With a FusedAdamW attached whose gradient buffer was just zeroed (the trainer's zero_grad -> backward order,
    train.py:186-192) the views are the optimizer's own `.grad` slots: the kernels write the gradients in place and the
    ~120 per-parameter AccumulateGrad additions of autograd disappear.  Otherwise (no fused optimizer, or a second
    backward without zero_grad = gradient accumulation) a scratch buffer is returned and autograd accumulates as usual.
    scratch=True (backward passes pre-launched inside training_step, i.e. BEFORE the trainer's zero_grad): the optimizer's
    persistent scratch buffer in the same padded layout; _finish_backward() moves it into `.grad` with one kernel."""
    if fused is not None and scratch:      # scratch: True, or the generation training_step() claimed on the caller's thread
        views = fused.scratch_views(plist, bump=scratch is True)
        if views is not None:
            return fused.scratch, views, ('scratch', fused.scratch_gen if scratch is True else int(scratch))
    if fused is not None and not scratch:
        views = fused.claim_fresh_grads(plist)
        if views is not None:
            return fused.flat_grad, views, True
    # zeros, not empty: a parameter no kernel of the pass writes (the auxiliary ActorCritic's actor, dreamer.py:347-358) would
    # otherwise hand autograd whatever the allocator's block held before
    flat = torch.zeros(sum(p.numel() for p in plist), device=device)
    views, off = [], 0
    for p in plist:
        views.append(flat[off:off + p.numel()].view(p.shape))
        off += p.numel()
    return flat, views, False


def _check_shapes(want, got):
    """The C side sizes every access from the geometry alone: refuse what the caller handed over in another shape."""
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    if bad:
        raise ValueError('training_step input shapes (got, expected): ' + ', '.join(f'{k}: {v[0]} != {v[1]}' for k, v in bad.items()))


def _grow_ws(buf, need, device):
    """`buf` when it holds `need` bytes on `device`, else a new workspace of that size."""
    if buf is None or buf.numel() < need or buf.device != device:
        buf = torch.empty(need, dtype=torch.uint8, device=device)
    return buf


def _cat_target_index(x, NE, C, cells):
    """The (NE, cells) int32 class index of a categorical target: target.argmax(dim=-3) (decoders.py:221) of a float one-hot
    (..., C, S, S); an integer class map (..., S, S) is taken as it is."""
    if not x.is_floating_point():
        return x.to(torch.int32).contiguous().view(NE, cells)
    target = torch.empty(NE, cells, dtype=torch.int32, device=x.device)
    H.call('dm_cat_target_index', NE, C, cells, H.fptr(x.float().contiguous()), H.ptr(target), H.stream())
    return target


def _multi_sum(items, device, out=None):
    """items: list of (tensor, scale) or (tensor, scale, center_tensor[, mode]) -> 1-D tensor of results (written into `out`,
    a slice of the step's metric buffer, when given)."""
    arr = (H.dm_reduce_item * len(items))()
    for i, it in enumerate(items):
        arr[i].x = it[0].data_ptr()
        arr[i].n = it[0].numel()
        arr[i].scale = it[1]
        if len(it) > 2:
            arr[i].mode = it[3] if len(it) > 3 else 1
            arr[i].center = it[2].data_ptr()
        else:
            arr[i].mode = 0
            arr[i].center = None
    if out is None:
        out = torch.empty(len(items), device=device)
    assert out.numel() == len(items) and out.is_contiguous()
    H.call('dm_multi_sum', len(items), arr, H.fptr(out), H.stream())
    return out


# One device buffer per step for every loss / metric scalar: slot layout
METRIC_SLOTS = dict(loss_kl=0, loss_image=1, loss_reward=2, loss_terminal=3, entropy_prior=4, entropy_post=5, loss_model=6,
                    loss_critic=8, loss_actor=9, policy_entropy=10, policy_value=11, policy_value_im=12, policy_reward=13,
                    policy_reward_std=14, grad_norm=16, grad_norm_probe=18, grad_norm_actor=20, grad_norm_critic=22,
                    loss_critic_aux=24, policy_value_aux=25, loss_vecobs=15,      # slot 7: loss_model + aux_critic_weight * loss_critic_aux
                    loss_map=28, acc_map=29, acc_map_seen=30)      # the map probe's (MapProbeHead); zero with probe_model='none'
# the goals probe's ten scalars (GoalsProbe): appended behind METRIC_SLOTS, named by packed_metrics() only for a model that has a
# goals probe, zero otherwise.  Slots 34-41 are the eight floats dm_goals_stats writes.
GOALS_STAT_NAMES = ('mse_goals', 'var_goals') + tuple(f'mse_goal_age{a}' for a in (0, 5, 10, 50, 200, 1000))
GOALS_METRIC_SLOTS = {k: 32 + i for i, k in enumerate(('loss_goal_direction', 'loss_goals_direction') + GOALS_STAT_NAMES)}
METRIC_BUF_FLOATS = 48
# the percentile return normalisation's three scalars (ActorCritic, return_norm='percentile'): free slots behind the goals probe's,
# named by packed_metrics() only for a model that has the switch on, zero otherwise (dm_return_norm's out[2:5], copied on the device)
RETURN_METRIC_SLOTS = dict(policy_return_lo=42, policy_return_hi=43, policy_return_scale=44)
# free bits' two scalars (WorldModel, kl_free > 0): the free slots behind those, named by packed_metrics() only for a model that has
# the switch on, zero otherwise.  loss_kl_clip: the mean of max(kl_free, kl) per row, the value loss_model is combined from;
# kl_free_frac: the fraction of closed rows (kl <= kl_free).  Slot 47 stays free
KL_FREE_METRIC_SLOTS = dict(loss_kl_clip=45, kl_free_frac=46)
CRITIC_DISTS = ('mse', 'twohot')
RETURN_NORMS = ('none', 'percentile')
# the config keys Dreamer hands to its task ActorCritic under the same names (a conf without them - an older namespace - gets the
# constructor's defaults).  The auxiliary critic and Plan2Explore's exploration ActorCritic keep the defaults
AC_CONF_KEYS = ('critic_dist', 'critic_bins', 'critic_bin_range', 'return_norm', 'return_norm_lo', 'return_norm_hi',
                'return_norm_decay', 'return_norm_limit')


def _finish_backward(owner, grads, flat, direct, grad_loss):
    """Chain rule with the incoming scalar gradient (1.0 unless a GradScaler is active) without a host sync, and hand-over
    of the gradients: returns the tuple for autograd (None when they already sit in the optimizer's `.grad` slots)."""
    gl = grad_loss.detach().float().reshape(1).contiguous()
    fused = getattr(owner, '_fused', None)
    if fused is not None and flat is fused.scratch:
        if not isinstance(direct, tuple) or direct[1] != fused.scratch_gen:
            raise RuntimeError('the gradients pre-computed by this training_step() were overwritten by a later training_step() '
                               'before backward() was called; call backward() after each training_step(), or set '
                               'model.overlap_backward = False to compute gradients inside backward()')
        fused.order_after_current()          # (pipelined mode: `gl` was made on this stream, the hand-over runs on the group's)
        if fused.home is not None:
            gl.record_stream(fused.home)
        fused.adopt_scratch(gl)              # buffer swap ('=' semantics) or accumulation; see FusedAdamW.adopt_scratch
        return tuple(None for _ in grads)
    H.call('dm_scale_inplace', H.fptr(flat), flat.numel(), H.fptr(gl), H.stream())
    return tuple(None for _ in grads) if direct else tuple(grads)


_HEADS_EARLY = True     # A/B switch: False runs the heads over the imagined states behind the rollout only
_WGRAD_SIDE = True      # A/B switch: False keeps every weight gradient on the caller's stream


def _warn_if_communicator_exists():
    """The step's streams are about to be created: has torch's default process group built its RCCL communicator already?"""
    try:
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_backend() != 'nccl':
            return
        be = dist.distributed_c10d._get_default_group()._get_backend(torch.device('cuda'))
        if be._is_initialized():
            import warnings
            warnings.warn('pydreamer_amd: an RCCL communicator exists before the model\'s streams were created - every training step '
                          'will be slower by 10-20 ms (hardware-queue assignment order; profiles/r06_force_dp.txt).  Build the model and '
                          'call init_optimizers() / prepare_streams() before the first collective.', RuntimeWarning, stacklevel=3)
    except Exception:       # a diagnostic only: private torch API
        pass


class _Overlap:
    """Side streams for the backward passes.  Everything the three backward passes consume is fixed once the matching
    forward has run (dreamer.py:149-157 detaches the features the actor-critic trains on), so training_step() launches
      * the world-model backward (decoder / heads, the strictly sequential BPTT chain of T x ~9 small kernels that
        leaves most of the 256 CUs idle, encoder) on `s_wm` right after the world-model forward, concurrently with the
        imagination rollout and the actor-critic forward on the caller's stream, and
      * the actor / critic backward on `s_ac` right after their forward.
    They write into the optimizers' scratch buffers (the trainer calls zero_grad() between training_step() and
    backward(), train.py:186-192); loss.backward() joins the stream and moves the result into `.grad`, so callers see
    ordinary stream semantics.  Each stream has its own workspace."""

    def __init__(self, device):
        # the latency-bound chain gets the high-priority queue: its 40-110-workgroup kernels must be dispatched ahead of
        # the thousands of queued GEMM workgroups of the concurrent work, or the chain just slows down
        self.s_wm = torch.cuda.Stream(device, priority=-1)
        self.s_ac = torch.cuda.Stream(device)
        self.ev_wm_fwd = torch.cuda.Event()
        self.ev_fwd = torch.cuda.Event()
        self.ev_fork, self.ev_tail = torch.cuda.Event(), torch.cuda.Event()      # the world-model forward's tail on s_wm (WorldModel._forward)
        # the rollout's progress mark (recorded by the library, dm_dream_rollout_marks) and the early head window's completion
        self.ev_mark, self.ev_heads = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.device(device):
            self.ev_mark.record()          # (torch creates the HIP event at the first record; the library needs its handle)
            self.ev_heads.record()
        # Every stream of the step gets one command NOW (round 6): a HIP stream takes its hardware queue when it first gets work, and
        # which streams later SHARE a queue depends on that order - a communicator created before these streams had run anything
        # cost the step +13 ms, a communicator that appeared mid-step +6 ms (profiles/r06_force_dp.txt).
        with torch.cuda.device(device):
            for st in (self.s_wm, self.s_ac):
                with torch.cuda.stream(st):
                    torch.zeros(64, device=device)
            if _WGRAD_SIDE:
                try:
                    H.call('dm_wgrad_side_touch')
                except H.DreamerHipError:       # an optimisation only (the library owns ONE side stream, on the device that used it first)
                    pass
            torch.cuda.synchronize(device)
        self.ws_wm = None
        self.ws_ac = None
        # The HIP runtime needs ~6 us of host time per kernel launch and a step is ~1800 launches; at small per-GPU
        # batches (data parallel: B/8 rows) the step is bound by exactly that.  The pre-launched backward passes are
        # therefore ENQUEUED by a second host thread (ctypes drops the GIL inside the C calls), in parallel with the
        # caller's thread enqueuing the imagination rollout.
        self.device = device
        self.pool = None

    def submit(self, stream, wait_event, fn):
        """Run fn() on `stream` (after `wait_event`) from the launcher thread; returns a Future."""
        if torch.cuda.is_current_stream_capturing():      # graph capture is bound to the capturing thread
            stream.wait_event(wait_event)
            with torch.cuda.stream(stream):
                return _Done(fn())
        if self.pool is None:
            import concurrent.futures
            self.pool = concurrent.futures.ThreadPoolExecutor(max_workers=1, thread_name_prefix='dm-launch')

        def job():
            with torch.cuda.device(self.device), torch.no_grad():
                stream.wait_event(wait_event)
                with torch.cuda.stream(stream):
                    return fn()
        return self.pool.submit(job)


def pack_metrics(*dicts):
    """the trainer reads ~20 scalar metrics per logged step with one `.item()` (= one device sync) each
    (train.py:204-214).  All metrics of this package are 0-d device tensors produced without a sync; this packs any
    number of metric dicts into ONE 1-D device tensor so a single `.cpu()` / non-blocking copy replaces the syncs:
        names, packed = pack_metrics(loss_metrics, grad_metrics);  values = dict(zip(names, packed.tolist()))"""
    names, vals = [], []
    for d in dicts:
        for k, v in d.items():
            names.append(k)
            vals.append(v.detach().reshape(()).float())
    return names, (torch.stack(vals) if vals else torch.empty(0))


class _Thunk:
    __slots__ = ('fn',)

    def __init__(self, fn):
        self.fn = fn


class LazyTensors(dict):
    """The `tensors` dict of training_step() (train.py:218-221 logs it only when `will_log_batch`): values may be thunks
    that are computed - and cached - the first time somebody reads them.  `image_rec` (123 MB at Atari-literal,
    decoders.py:177) is the one that matters: it is no longer written on the steps that never look at it."""

    def _resolve(self, k, v):
        if isinstance(v, _Thunk):
            v = v.fn()
            dict.__setitem__(self, k, v)
        return v

    def lazy(self, k, fn):
        dict.__setitem__(self, k, _Thunk(fn))

    def __getitem__(self, k):
        return self._resolve(k, dict.__getitem__(self, k))

    def __iter__(self):                     # overriding __iter__ also keeps dict(x) / {**x} off CPython's raw-copy fast path
        return iter(list(dict.keys(self)))

    def get(self, k, default=None):
        return self[k] if k in self else default

    def items(self):
        return [(k, self[k]) for k in dict.keys(self)]

    def values(self):
        return [self[k] for k in dict.keys(self)]

    def pop(self, k, *default):
        if k in self:
            v = self[k]
            dict.__delitem__(self, k)
            return v
        if default:
            return default[0]
        raise KeyError(k)

    def copy(self):
        new = LazyTensors()
        for k in dict.keys(self):
            dict.__setitem__(new, k, dict.__getitem__(self, k))      # thunks stay thunks
        return new

    def is_materialised(self, k):
        return not isinstance(dict.__getitem__(self, k), _Thunk)


class _Done:
    def __init__(self, value):
        self.value = value

    def result(self):
        return self.value


def _require_cuda(t, what):
    if not t.is_cuda:
        raise H.DreamerHipError(f'{what} is on {t.device}: pydreamer_amd has no CPU path (the HIP library is the product)')


# ---------------------------------------------------------------------------------------------------------------
# world model
# ---------------------------------------------------------------------------------------------------------------
class _WMStep(torch.autograd.Function):
    """loss_model = WorldModel forward; backward = hand-written BPTT + conv backward through the C-ABI."""

    @staticmethod
    def forward(ctx, wm, pack, *params):
        ctx.wm, ctx.pack = wm, pack
        tail = pack.get('tail')
        if tail is not None:                  # the loss was written on the world-model stream (WorldModel._forward)
            with torch.cuda.stream(tail.s_wm):
                return pack['loss'].clone()
        return pack['loss'].clone()

    @staticmethod
    def backward(ctx, grad_loss):
        wm, pk = ctx.wm, ctx.pack
        if pk.get('consumed'):
            raise RuntimeError('loss_model.backward() called twice (saved activations were released)')
        ov = pk.get('overlap')
        if 'pre' in pk:                                   # launched on s_wm inside training_step()
            grads, flat, direct = pk.pop('pre').result()
            torch.cuda.current_stream().wait_stream(ov.s_wm)
        else:
            grads, flat, direct = wm._backward(pk, pk['ws'])
        for k in ('enc_acts', 'rssm_acts', 'dec_acts', 'heads', 'aux', 'ev_acts', 'enc_x', 'dlogits'):
            pk.pop(k, None)                               # only now: the side stream may have been reading them
        pk['consumed'] = True
        return (None, None) + _finish_backward(wm, grads, flat, direct, grad_loss)


def open_loop_struct(cell):
    """rssm.py:50-53: every step is RSSMCell.forward_prior - the same trunk, then the PRIOR head on h' with no embedding term.
    That is dm_rssm_sequence_fwd with the posterior head's parameter slots pointing at the prior head and a zero embedding (its
    product with post_mlp_e is then an exact zero).  Forward only.  Used by WorldModel._forward(open_loop=True) and by the
    planner's candidate rollout (planner.CEMPlanner)."""
    po = list(cell.ordered())
    ix = {n: i for i, n in enumerate(H.RSSM_PARAM_ORDER)}
    for dst, src in (('post_mlp_h.weight', 'prior_mlp_h.weight'), ('post_mlp_h.bias', 'prior_mlp_h.bias'),
                     ('post_norm.weight', 'prior_norm.weight'), ('post_norm.bias', 'prior_norm.bias'),
                     ('post_mlp.weight', 'prior_mlp.weight'), ('post_mlp.bias', 'prior_mlp.bias')):
        po[ix[dst]] = po[ix[src]]
    return H.rssm_struct(po)


class WorldModel(_Params):
    """dreamer.py:228-396."""

    def __init__(self, conf):
        super().__init__()
        if conf.aux_critic and conf.iwae_samples != 1:
            raise NotImplementedError('aux_critic assumes iwae_samples = 1 (as the reference does, dreamer.py:349)')
        self.dense = dense_image_gate(conf)      # the dense categorical image path instead of the convolution stacks
        # no image at all: image_size, image_channels and cnn_depth are not read on that path
        self.imageless = not self.dense and imageless_gate(conf)
        if not self.dense and not self.imageless and conf.image_size != 64:
            raise NotImplementedError('conv geometry is built for 64x64 observations')
        self.conf = conf
        self.deter_dim, self.stoch_dim, self.stoch_discrete = conf.deter_dim, conf.stoch_dim, conf.stoch_discrete
        self.kl_weight = conf.kl_weight
        self.kl_balance = None if conf.kl_balance == 0.5 else conf.kl_balance     # dreamer.py:241
        # free bits per (t, b) row, in nats (DreamerV3's rule; 0: off, the reference's loss): max(kl_free, kl) enters loss_model and a
        # row with kl <= kl_free sends no gradient into post or prior (dm_kl_free_fwd / dm_kl_free_bwd)
        self.kl_free = float(getattr(conf, 'kl_free', 0.0))
        if not (math.isfinite(self.kl_free) and self.kl_free >= 0.0):
            raise ValueError(f'kl_free={self.kl_free!r}: a finite number of nats >= 0')
        if self.kl_free > 0 and conf.iwae_samples > 1:
            raise NotImplementedError('kl_free > 0 with iwae_samples > 1: the sampled KL of the IWAE bound has no per-row exact KL '
                                      'to clip')
        self.aux_critic_weight = conf.aux_critic_weight
        self.encoder = MultiEncoder(conf)
        features_dim = conf.deter_dim + conf.stoch_dim * (conf.stoch_discrete or 1)
        self.features_dim = features_dim
        self.decoder = MultiDecoder(features_dim, conf)
        self.core = RSSMCore(embed_dim=self.encoder.out_dim, action_dim=conf.action_dim, deter_dim=conf.deter_dim,
                             stoch_dim=conf.stoch_dim, stoch_discrete=conf.stoch_discrete, hidden_dim=conf.hidden_dim,
                             gru_layers=conf.gru_layers, gru_type=conf.gru_type, layer_norm=conf.layer_norm)
        # Auxiliary critic on the real trajectory (dreamer.py:267-279): a full ActorCritic lives inside the world model (its
        # parameters belong to the world-model optimizer and get the tf2 init); only its critic is trained (dreamer.py:347-358)
        self.ac_aux = None
        if conf.aux_critic:
            self.ac_aux = ActorCritic(in_dim=features_dim, out_actions=conf.action_dim, layer_norm=conf.layer_norm,
                                      gamma=conf.gamma_aux, lambda_gae=conf.lambda_gae_aux, entropy_weight=conf.entropy,
                                      target_interval=conf.target_interval_aux, actor_grad=conf.actor_grad,
                                      actor_dist=conf.actor_dist)
        for m in self.modules():
            init_weights_tf2(m)
        for m in self.modules():      # (behind the initialiser above, which fills every Linear: a head that wants a zero output layer)
            if hasattr(m, 'zero_output'):
                m.zero_output()
        self._ws = None
        self._ws_dec = None                # own workspaces of the decoder / encoder backward while weight gradients are deferred
        self._ws_enc = None

    def init_state(self, batch_size):
        return self.core.init_state(batch_size)

    # ---- shape / workspace
    def shape(self, T, B, H_):
        c = self.conf
        return H.make_shape(T=T, B=B, I=1, H=H_, D=c.deter_dim, Hd=c.hidden_dim, S=c.stoch_dim, C=c.stoch_discrete,
                            E=self.encoder.out_dim, A=c.action_dim, mlp_hidden=MLP_HIDDEN, mlp_layers=4,
                            # (dense: no convolution scratch in dm_workspace_bytes; image-less: no image geometry at all)
                            cnn_depth=0 if self.imageless else 1 if self.dense else c.cnn_depth,
                            img=0 if self.imageless else c.image_size, img_ch=0 if self.imageless else c.image_channels,
                            flags=ACTOR_KINDS.get(c.actor_dist, 0) | (H.GRU_KINDS[c.gru_type] << H.DM_FLAG_GRU_SHIFT) |
                            ((c.gru_layers - 1) << H.DM_FLAG_GRU_LAYERS_SHIFT) |
                            (H.DM_FLAG_BF16 if getattr(c, 'amp', False) else 0))

    def workspace(self, shp, device):
        need = H.workspace_bytes(shp)
        if self.dense:      # the image MLPs may be deeper than the four layers dm_workspace_bytes sizes the heads for
            deep = max(4, self.encoder.encoder_image.hidden_layers, self.decoder.image.hidden_layers)
            need = max(need, 4 * int(H.lib().dm_mlp_ws_floats(shp.T * shp.B * max(shp.I, 1), MLP_HIDDEN, deep)))
        self._ws = _grow_ws(self._ws, need, device)
        return self._ws

    def forward(self, obs, in_state, u_post=None):
        """dreamer.py:289-295: features and out_state only (used by Dreamer.inference)."""
        with torch.no_grad():
            pk = self._forward(obs, in_state, u_post, None, forward_only=True)
        T, B = obs['action'].shape[:2]
        return pk['feat'].view(T, B, 1, -1), pk['out_state']

    # ---- forward through the C-ABI
    def _forward(self, obs, in_state, u_post, forced_idx, forward_only=False, imag_horizon=1, open_loop=False, mbuf=None,
                 iwae=1, tail=None):
        """iwae = I > 1 (rssm.py:35-41): every row-wise stage runs on T*B*I rows, row n = (t*B + b)*I + i; only the conv
        encoder sees the T*B frames once.  Three geometry structs: `shp` (T,B,I: conv decoder + workspace), `shp_e`
        (T,B,1: encoder), `shp_r` (T, B*I, 1: the RSSM calls take the expanded batch as their batch)."""
        c = self.conf
        action = obs['action']
        # the step's device is the image's; image-less the action's
        src = 'action' if self.imageless else 'image'
        _require_cuda(obs[src], f"obs['{src}']")
        T, B = action.shape[:2]
        I = int(iwae)
        BI = B * I
        N, dev = T * B * I, obs[src].device
        D_, F_, E = c.deter_dim, self.features_dim, self.encoder.out_dim
        gauss = not c.stoch_discrete         # Gaussian latents: z is stoch_dim wide, its parameters (mean | raw std) twice that
        Z, ZP = c.stoch_dim * (c.stoch_discrete or 1), c.stoch_dim * (c.stoch_discrete or 2)
        if gauss and forced_idx is not None:
            raise NotImplementedError('Gaussian latents (stoch_discrete=0) have no indices to force')
        shp = self.shape(T, B, imag_horizon)
        shp.I = I
        ws = self.workspace(shp, dev)
        action = action.float().contiguous()
        reset = obs['reset'].to(torch.uint8).contiguous()
        h0, z0 = (x.float().contiguous() for x in in_state)
        # the C side sizes every access from dm_shape alone: check what the caller handed over before packing pointers (this
        # model's own entries; the encoder adds what it reads and runs the check)
        want = dict(action=(T, B, c.action_dim), reset=(T, B))
        got = dict(action=tuple(action.shape), reset=tuple(reset.shape))
        for k in ('reward', 'terminal'):
            if k in obs:
                want[k], got[k] = (T, B), tuple(obs[k].shape)
        want['in_state[0]'], got['in_state[0]'] = (BI, D_), tuple(h0.shape)
        want['in_state[1]'], got['in_state[1]'] = (BI, Z), tuple(z0.shape)
        if u_post is not None:
            want['u_post numel'], got['u_post numel'] = T * BI * c.stoch_dim, u_post.numel()
        if forced_idx is not None:
            want['forced_idx'], got['forced_idx'] = (T, BI, c.stoch_dim), tuple(forced_idx.shape)
        image, _, plane_r, plane_t, vecobs = self.encoder.ingest(obs, T, B, shp, want, got)
        # Every buffer of the step is its own allocation: nothing is shared between steps, so a backward() on an older
        # step's losses is always valid.  Uniforms for the categorical inverse-CDF rule; standard-normal eps of
        # Normal.rsample for Gaussian latents.
        if u_post is not None:
            u_post = u_post.reshape(T, BI, c.stoch_dim).float().contiguous()
        elif forced_idx is None:
            u_post = (torch.randn if gauss else torch.rand)(T, BI, c.stoch_dim, device=dev)
        lib = H.lib()
        shp_e = shp_r = shp
        if I > 1:
            shp_e = H.dm_shape.from_buffer_copy(shp)
            shp_e.I = 1
            shp_r = H.dm_shape.from_buffer_copy(shp)
            shp_r.B, shp_r.I = BI, 1

        cell = self.core.cell
        rssm_p = H.rssm_struct(cell.ordered())
        if open_loop:
            rssm_p = open_loop_struct(cell)
        rssm_acts = torch.empty(int(lib.dm_rssm_acts_floats(ctypes.byref(shp_r))), device=dev)
        feat = torch.empty(N, F_, device=dev)
        post = torch.empty(N, ZP, device=dev)
        prior = torch.empty(N, ZP, device=dev)
        idx = torch.empty(N, c.stoch_dim, dtype=torch.int32, device=dev)
        fidx = forced_idx.to(torch.int32).contiguous() if forced_idx is not None else None
        u_ptr = H.fptr(u_post) if u_post is not None else None
        dec = self.decoder
        dec_acts = loss_image = None
        if not forward_only:
            dec_acts, loss_image = dec.image_buffers(shp, N, dev)

        # rssm.py:35-41: (T,B,X) -> (T,B*I,X), pure data movement (I = 1: the caller's tensors as they are)
        A_ = c.action_dim
        if I > 1:
            action_x = torch.empty(T, BI, A_, device=dev)
            action_x.view(T, B, I, A_).copy_(action.view(T, B, 1, A_).expand(T, B, I, A_))
            reset_x = torch.empty(T, BI, dtype=torch.uint8, device=dev)
            reset_x.view(T, B, I).copy_(reset.view(T, B, 1).expand(T, B, I))
        else:
            action_x, reset_x = action, reset
        embed, enc_st = self.encoder.encode(image, plane_r, plane_t, vecobs, shp_e, ws, forward_only)
        embed_x = embed
        if I > 1:
            embed_x = torch.empty(N, E, device=dev)
            embed_x.view(T, B, I, E).copy_(embed.view(T, B, 1, E).expand(T, B, I, E))
        embed_rssm = torch.zeros_like(embed_x) if open_loop else embed_x
        H.call('dm_rssm_sequence_fwd', ctypes.byref(shp_r), H.fptr(embed_rssm), H.fptr(action_x), H.ptr(reset_x), H.fptr(h0),
               H.fptr(z0), u_ptr, H.ptr(fidx), ctypes.byref(rssm_p), H.fptr(rssm_acts), H.fptr(feat), H.fptr(post),
               H.fptr(prior), H.ptr(idx), H.ptr(ws), ws.numel(), H.stream())

        last = feat[(T - 1) * BI:]
        out_state = (last[:, :D_].clone(), last[:, D_:].clone())                  # detached by construction (rssm.py:77)
        pk = dict(shp=shp, shp_r=shp_r, T=T, B=B, I=I, feat=feat, post=post, prior=prior, idx=idx,
                  out_state=out_state, embed_x=embed_x, action_x=action_x, reset_x=reset_x, **enc_st)
        if forward_only:
            return pk
        # The tail of the world-model forward - decoder + MSE, reward / terminal heads, KL, the loss sums (dreamer.py:311-365) -
        # is consumed by the world-model BACKWARD only: the imagination rollout (dreamer.py:149-157) needs the posterior
        # features and nothing else.  With `tail` (the training step's side streams, Dreamer.training_step) it is enqueued on
        # the world-model stream, in front of the pre-launched backward, with that stream's workspace, and the caller's stream
        # goes from the posterior loop straight to the rollout.  Same kernels on the same operands: bit-identical
        # (test_world_model_tail_on_side_stream_is_bit_identical).
        use_tail = tail is not None
        if use_tail:
            ws = tail.ws_wm = _grow_ws(tail.ws_wm, ws.numel(), dev)
            tail.ev_fork.record(torch.cuda.current_stream())
            tail.s_wm.wait_event(tail.ev_fork)
            pk['tail'] = tail
        with (torch.cuda.stream(tail.s_wm) if use_tail else contextlib.nullcontext()):
            return self._forward_tail(pk, obs, c, dec, dec_acts, loss_image, ws, mbuf, action, reset, rssm_acts)

    def _forward_tail(self, pk, obs, c, dec, dec_acts, loss_image, ws, mbuf, action, reset, rssm_acts):
        shp, T, B, I, feat, post, prior, idx = (pk[k] for k in ('shp', 'T', 'B', 'I', 'feat', 'post', 'prior', 'idx'))
        N, NE, dev = T * B * I, T * B, feat.device
        D_, F_, gauss = c.deter_dim, self.features_dim, not c.stoch_discrete
        # gw: the data-parallel shard weight B_r/B (dist.attach), folded into every gradient scale; loss values are unaffected
        gw = float(getattr(self, 'grad_weight', 1.0))
        pk.update(dec.image_loss(shp, feat, pk['image'], ws, dec_acts, loss_image, gw))
        heads, pk['heads'] = dec.heads_loss(pk, obs, ws, gw)      # name -> (loss, rec, target) per row; the backward's entries
        # KL + entropies (dreamer.py:326-343,369-379)
        kl, ent_post, ent_prior = (torch.empty(N, device=dev) for _ in range(3))
        free = self.kl_free > 0
        if free:
            kl_clip, closed = torch.empty(N, device=dev), torch.empty(N, device=dev)
            H.call('dm_kl_free_fwd', N, c.stoch_dim, c.stoch_discrete, H.fptr(post), H.fptr(prior), self.kl_free, H.fptr(kl),
                   H.fptr(kl_clip), H.fptr(closed), H.fptr(ent_post), H.fptr(ent_prior), H.stream())
            pk['closed'] = closed
        else:
            H.call('dm_kl_balance_fwd', N, c.stoch_dim, c.stoch_discrete, H.fptr(post), H.fptr(prior), H.fptr(kl),
                   H.fptr(ent_post), H.fptr(ent_prior), H.stream())

        if mbuf is None:
            mbuf = torch.zeros(METRIC_BUF_FLOATS, device=dev)
        loss, iw, aux = mbuf[6], None, None
        if self.ac_aux is not None and T >= 2:
            # Auxiliary critic (dreamer.py:347-358): ActorCritic.training_step on the REAL trajectory - features (T,B,F) as
            # the "dream", the batch's own actions / rewards / terminals; only loss_critic is kept.  Its actor forward and
            # policy loss are computed by the reference and then thrown away, so they are simply not run here.
            ac = self.ac_aux
            # a2c.py:76-79 via dreamer.py:349: ac_aux.training_step runs with log_only=False also under no_grad evaluation,
            # so the target refresh and the counter advance on EVERY call (the reference's behaviour, mirrored)
            if ac.train_steps % ac.target_interval == 0:
                ac.update_critic_target()
            ac.train_steps += 1
            rows = (T - 1) * B
            value_t, _ = ac.critic_target.fwd(feat, F_, N, ws, save_acts=False, sparse_cols=dec.sparse_cols)
            value, aux_acts = ac.critic.fwd(feat, F_, N, ws, sparse_cols=dec.sparse_cols)
            adv, agae, vtgt, wgt = (torch.empty(T - 1, B, device=dev) for _ in range(4))
            H.call('dm_gae_losses', T - 1, B, ac.gamma, ac.lambda_, H.fptr(heads['reward'][2]), H.fptr(heads['terminal'][2]), H.fptr(value_t),
                   H.fptr(adv), H.fptr(agae), H.fptr(vtgt), H.fptr(wgt), H.stream())
            lc = torch.empty(rows, device=dev)
            dvalue = torch.zeros(N, device=dev)                      # value[-1] gets no gradient
            H.call('dm_critic_loss', rows, H.fptr(value), H.fptr(vtgt), H.fptr(wgt), gw * self.aux_critic_weight / rows, H.fptr(lc),
                   H.fptr(dvalue), H.stream())
            _multi_sum([(lc, 1.0 / rows), (value.view(T, B)[:-1], 1.0 / rows)], dev, out=mbuf[24:26])
            aux = dict(acts=aux_acts, dvalue=dvalue, value=value, lc=lc, rows=rows)
        # loss_model = mean_tb of the weighted terms [kl, image (none on the image-less path), *heads] (dreamer.py:362-365)
        names = list(heads)
        img = [] if loss_image is None else [(loss_image, dec.image_weight)]
        xs = [kl_clip if free else kl] + [x for x, _ in img] + [heads[n][0] for n in names]
        wts = [self.kl_weight] + [w for _, w in img] + [w for _, _, w in dec.heads()]
        red = lambda x, mode: x
        if I > 1:
            # IWAE: sampled KL (dreamer.py:340-343); loss_model = mean_tb -logavgexp_i(-loss_tbi) (dreamer.py:362-365);
            # the logged tensors are -logavgexp_i(-x) of the per-sample losses (decoders.py:170,277,312), means over I for the
            # entropies and the reconstructions (dreamer.py:371-372, decoders.py:171,278,313)
            xs[0] = torch.empty(N, device=dev)
            if gauss:      # Normal log-densities of the reparameterised sample z = feat[:, D:] (rssm.py:202-203)
                H.call('dm_kl_sampled_gauss_fwd', N, c.stoch_dim, H.fptr(post), H.fptr(prior),
                       ctypes.c_void_p(feat.data_ptr() + 4 * D_), F_, H.fptr(xs[0]), H.stream())
            else:
                H.call('dm_kl_sampled_fwd', N, c.stoch_dim, c.stoch_discrete, H.fptr(post), H.fptr(prior), H.ptr(idx), H.fptr(xs[0]),
                       H.stream())
            l_tbi = torch.empty(N, device=dev)
            ptrs = (ctypes.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
            H.call('dm_combine_rows', len(xs), N, ptrs, (ctypes.c_float * len(wts))(*wts), H.fptr(l_tbi), H.stream())
            iw = torch.empty(N, device=dev)                   # importance weights softmax_i(-loss_tbi) = d loss_tb / d loss_tbi
            l_tb = _reduce_i(l_tbi, NE, I, 1, iw=iw)
            red = lambda x, mode: _reduce_i(x, NE, I, mode)
        # Per (t,b), and the means in the metric buffer: slots 0-5 and under IWAE loss_model in slot 6 are one launch (image-less, an
        # item of zero elements leaves an exact 0.0 in slot 1); every further head has a slot of its own
        t_kl = red(kl, 1)
        t_li = None if loss_image is None else red(loss_image, 1)
        t_loss = {n: red(heads[n][0], 1) for n in names[:2]}
        t_ep, t_eq = red(ent_prior, 0), red(ent_post, 0)
        t_rec = {n: red(heads[n][1], 0) for n in names[:2]}
        items = [t_kl, torch.empty(0, device=dev) if t_li is None else t_li, *t_loss.values(), t_ep, t_eq] + ([l_tb] if I > 1 else [])
        _multi_sum([(x, 1.0 / NE) for x in items], dev, out=mbuf[0:len(items)])
        for n in names[2:]:
            t_loss[n], t_rec[n] = red(heads[n][0], 1), red(heads[n][1], 0)
            s = METRIC_SLOTS[f'loss_{n}']
            _multi_sum([(t_loss[n], 1.0 / NE)], dev, out=mbuf[s:s + 1])
        if I == 1:
            def combine(sums, w, slot):
                H.call('dm_combine', len(w), H.fptr(sums), (ctypes.c_float * len(w))(*w), ctypes.c_void_p(mbuf.data_ptr() + 4 * slot),
                       H.stream())
            terms = [(x, 1.0 / N) for x in xs]
            # (kl, image, reward, terminal and nothing else: their means stand in slots 0-3 already)
            # (free bits: slot 0 keeps the exact KL, the clipped mean is summed with the other terms)
            combine(mbuf[0:4] if img and not names[2:] and not free else _multi_sum(terms, dev), wts, 6)
            if aux is not None:       # loss = loss_model.mean() + aux_critic_weight * loss_critic_aux (dreamer.py:365) -> slot 7
                combine(_multi_sum(terms + [(aux['lc'], 1.0 / aux['rows'])], dev), wts + [self.aux_critic_weight], 7)
                loss = mbuf[7]

        pk.update(loss=loss, action=action, reset=reset, rssm_acts=rssm_acts, ws=ws, mbuf=mbuf, iw=iw, aux=aux)
        tb = lambda x: x.view(T, B, *x.shape[1:])
        tensors = dict(loss_kl=tb(t_kl), entropy_prior=tb(t_ep), entropy_post=tb(t_eq))
        metrics = dict(loss_model=mbuf[6], loss_kl=mbuf[0], entropy_prior=mbuf[4], entropy_post=mbuf[5])
        if free:
            s0 = KL_FREE_METRIC_SLOTS['loss_kl_clip']
            _multi_sum([(kl_clip, 1.0 / N), (closed, 1.0 / N)], dev, out=mbuf[s0:s0 + 2])
            tensors['loss_kl_clip'] = tb(kl_clip)
            metrics.update({k: mbuf[i] for k, i in KL_FREE_METRIC_SLOTS.items()})
        if t_li is not None:      # (decoders.py:59-64: image-less there is no loss_image metric and no loss_image / image_rec tensor)
            tensors.update(loss_image=tb(t_li), image_rec=None)
            metrics.update(loss_image=mbuf[1])
        for n in names:
            tensors.update({f'loss_{n}': tb(t_loss[n]), f'{n}_rec': tb(t_rec[n])})
            metrics[f'loss_{n}'] = mbuf[METRIC_SLOTS[f'loss_{n}']]
        pk['tensors'], pk['metrics'] = LazyTensors(tensors), metrics
        if t_li is not None:
            pk['tensors'].lazy('image_rec', dec.image_rec_thunk(pk))
        if aux is not None:
            pk['metrics'].update(loss_critic_aux=mbuf[24], policy_value_aux=mbuf[25])
            pk['tensors']['policy_value_aux'] = aux['value'].view(T, B)
        return pk

    def _param_order(self):
        return list(self.parameters())

    def _backward(self, pk, ws, scratch=False, defer_wgrad=False):
        c = self.conf
        shp, T, B, I = pk['shp'], pk['T'], pk['B'], pk.get('I', 1)
        NE, N = T * B, T * B * I
        iw = pk.get('iw')          # IWAE importance weights (N,) or None: every per-sample gradient of loss_model carries them
        feat, dev = pk['feat'], pk['feat'].device
        F_, Z, E = self.features_dim, c.stoch_dim * (c.stoch_discrete or 2), self.encoder.out_dim   # Z: parameter width here
        plist = self._param_order()
        flat, views, direct = _flat_views(plist, dev, getattr(self, '_fused', None), scratch)
        gof = {id(p): v for p, v in zip(plist, views)}
        dec = self.decoder

        gw = float(getattr(self, 'grad_weight', 1.0))          # data-parallel shard weight B_r/B (dist.attach)
        dfeat = torch.zeros(N, F_, device=dev)
        # dense heads (decoders.py:73-83)
        if iw is not None and not pk.get('iw_applied'):
            for _, _, dout in pk['heads']:      # (N,) or (N, n): one importance weight per row
                n = dout.numel() // N
                H.call('dm_scale_rows', N, n, H.fptr(dout), n, H.fptr(iw), 1.0, H.stream())
            pk['iw_applied'] = True
        heads = list(pk['heads'])      # reward, terminal, vecobs (MultiDecoder.heads_loss)
        if pk.get('aux') is not None:          # the auxiliary critic trains on the world model's own features (not detached)
            heads.append((self.ac_aux.critic, pk['aux']['acts'], pk['aux']['dvalue']))
        heads += dec.image_heads(pk)
        for head, acts, dout in heads:
            head.bwd_into(gof, feat, F_, N, acts, dout, ws, dx=dfeat, lddx=F_, dx_accum=True)
        # Parameter gradients are leaves: nothing waits for them before the gradient clip, while the DATA gradients are the
        # chain decoder -> BPTT -> encoder.  Armed, the library enqueues the decoder's and the RSSM's parameter gradients on its
        # low-priority side stream, where they run beside the BPTT loop (a 50-row latency chain that leaves most CUs idle); they
        # read gradient buffers in the workspace of THEIR call, so each call gets its own (include/dreamer_hip.h
        # dm_wgrad_side_arm).  The encoder backward is not deferred (it is the tail: there is nothing left to hide behind).
        # (measured: no gain on a 7-column shard, -1.1 ms at 25 columns.  Rounds 3-5 switched it off under data parallelism, unmeasured;
        #  round 6 measured it over a one-rank RCCL group: off costs +0.9 ... +1.2 ms at 25 / 50 columns, on costs nothing beside the
        #  all-reduce - profiles/r06_force_dp.txt run K: it stays on there.)
        # (off on the dense and the image-less paths: no decoder call to hide the weight gradients behind, not measured there)
        side = defer_wgrad and _WGRAD_SIDE and B * I >= 16 and not torch.cuda.is_current_stream_capturing() and \
            not self.dense and not self.imageless
        ws_dec = ws_enc = ws
        if side:
            need = H.workspace_bytes(shp)
            ws_dec = self._ws_dec = _grow_ws(self._ws_dec, need, dev)
            ws_enc = self._ws_enc = _grow_ws(self._ws_enc, need, dev)      # decoder / BPTT (`ws`) / encoder: one each until the join
            H.call('dm_wgrad_side_arm', 1)
        try:
            dec.image_bwd(pk, gof, dfeat, gw * dec.image_weight / NE, iw, ws_dec)      # (convolution path; dense: a head above)
            # KL (dreamer.py:334-343)
            dpost = torch.empty(N, Z, device=dev)
            dprior = torch.empty(N, Z, device=dev)
            if iw is not None and not c.stoch_discrete:      # sampled Normal KL: explicit parameter gradients + the path through z
                D_ = c.deter_dim
                H.call('dm_kl_sampled_gauss_bwd', N, c.stoch_dim, H.fptr(pk['post']), H.fptr(pk['prior']),
                       ctypes.c_void_p(feat.data_ptr() + 4 * D_), F_, gw * self.kl_weight / NE, H.fptr(iw), H.fptr(dpost),
                       H.fptr(dprior), ctypes.c_void_p(dfeat.data_ptr() + 4 * D_), F_, H.stream())
            elif iw is not None:         # sampled KL of the IWAE bound
                H.call('dm_kl_sampled_bwd', N, c.stoch_dim, c.stoch_discrete, H.fptr(pk['post']), H.fptr(pk['prior']),
                       H.ptr(pk['idx']), gw * self.kl_weight / NE, H.fptr(iw), H.fptr(dpost), H.fptr(dprior), H.stream())
            else:
                if self.kl_balance is None:
                    sp = sq = gw * self.kl_weight / N
                else:
                    sp, sq = gw * self.kl_weight * (1 - self.kl_balance) / N, gw * self.kl_weight * self.kl_balance / N
                if self.kl_free > 0:      # closed rows (kl <= kl_free): exact zeros; open rows: the values of the call below
                    H.call('dm_kl_free_bwd', N, c.stoch_dim, c.stoch_discrete, H.fptr(pk['post']), H.fptr(pk['prior']),
                           H.fptr(pk['closed']), sp, sq, H.fptr(dpost), H.fptr(dprior), H.stream())
                else:
                    H.call('dm_kl_balance_bwd', N, c.stoch_dim, c.stoch_discrete, H.fptr(pk['post']), H.fptr(pk['prior']), sp, sq,
                           H.fptr(dpost), H.fptr(dprior), H.stream())
            # RSSM BPTT
            cell = self.core.cell
            rssm_p = H.rssm_struct(cell.ordered())
            rssm_g = H.rssm_struct([None if p is None else gof[id(p)] for p in cell.ordered()], cls=H.dm_rssm_grads)
            dembed = torch.empty(N, E, device=dev)
            H.call('dm_rssm_sequence_bwd', ctypes.byref(pk['shp_r']), H.fptr(pk['embed_x']), H.fptr(pk['action_x']),
                   H.ptr(pk['reset_x']), ctypes.byref(rssm_p), H.fptr(pk['rssm_acts']), H.fptr(feat), H.fptr(pk['post']),
                   H.fptr(dfeat), H.fptr(dpost), H.fptr(dprior), ctypes.byref(rssm_g), H.fptr(dembed), H.ptr(ws), ws.numel(),
                   H.stream())
            if I > 1:                  # the I samples of a (t,b) share one embedding row: their gradients add up
                dembed = _reduce_i(dembed, NE, I, 2)
            self.encoder.backward(dembed, pk, gof, ws_enc)
        except BaseException:
            if side:
                H.lib().dm_wgrad_side_join(H.stream())      # disarm this thread; the error propagates
            raise
        if side:
            H.call('dm_wgrad_side_join', H.stream())    # every gradient of this pass is complete on this stream from here on
        return views, flat, direct

    def _image_pred(self, pk, obs, u_pred):
        """do_image_pred (dreamer.py:381-394): decode from a PRIOR sample instead of the posterior sample and report the
        reconstruction losses as logprob_* / *_pred (decoders.py:50-108 with extra_metrics).  Logging variant, no grads.
        iwae_samples = I > 1 (the call shape of evaluate(), train.py:353-359,380-385): one prior sample per (t,b,i) row, which
        MultiDecoder.predict decodes and reduces TBI => TB."""
        c, dec = self.conf, self.decoder
        feat, shp, N, dev = pk['feat'], pk['shp'], pk['feat'].shape[0], pk['feat'].device
        D_, S, C, F_ = c.deter_dim, c.stoch_dim, c.stoch_discrete, self.features_dim
        ws = self.workspace(shp, dev)
        with torch.no_grad():
            if u_pred is None:
                u_pred = (torch.rand if C else torch.randn)(N, S, device=dev)
            u_pred = u_pred.reshape(N, S).contiguous()
            fp = feat.clone()                                                 # feature_replace_z: [h | prior sample]
            idx = torch.empty(N, S, dtype=torch.int32, device=dev)
            H.call('dm_sample_onehot', N, S, C, H.fptr(pk['prior']), S * (C or 2), H.fptr(u_pred), None,
                   ctypes.c_void_p(fp.data_ptr() + 4 * D_), F_, H.ptr(idx), H.stream())
            metrics, tensors = dec.predict(pk, fp, obs, ws)
        return metrics, tensors, idx

    def training_step(self, obs, in_state, iwae_samples=1, do_open_loop=False, do_image_pred=False, forward_only=False,
                      u_post=None, forced_idx=None, imag_horizon=1, u_pred=None, mbuf=None, _tail=None):
        """dreamer.py:297-396. Returns (loss, features (T,B,1,F), states, out_state, metrics, tensors)."""
        I = int(iwae_samples)
        if self.dense and I > 1:
            raise NotImplementedError('iwae_samples > 1 is not built on the dense image path (DESIGN 4.11)')
        if self.kl_free > 0 and I > 1:
            raise NotImplementedError('kl_free > 0 with iwae_samples > 1: the sampled KL has no per-row exact KL to clip')
        if do_open_loop and torch.is_grad_enabled():
            raise NotImplementedError('do_open_loop is an evaluation variant: call it under torch.no_grad() like '
                                      'train.py:353-359 does (its backward is not built)')
        T, B = obs['action'].shape[:2]
        if forward_only:
            feats, out_state = self.forward(obs, in_state)
            return torch.tensor(0.0), feats, None, out_state, {}, {}
        pk = self._forward(obs, in_state, u_post, forced_idx, imag_horizon=imag_horizon, open_loop=do_open_loop, mbuf=mbuf,
                           iwae=I, tail=None if (do_open_loop or do_image_pred) else _tail)
        loss = _WMStep.apply(self, pk, *self._param_order())
        if pk.get('tail') is not None:        # everything the forward's tail produced is final once the caller's stream has
            pk['tail'].ev_tail.record(pk['tail'].s_wm)      # waited for this event (Dreamer.training_step does, before returning)
        D_ = self.deter_dim
        feat = pk['feat']
        features = feat.view(T, B, I, -1)
        states = (feat[:, :D_].view(T, B, I, -1), feat[:, D_:].view(T, B, I, -1))
        self._last_pack = pk
        if do_image_pred:
            m, t, pk['pred_idx'] = self._image_pred(pk, obs, u_pred)
            pk['metrics'] = dict(pk['metrics'], **m)
            pk['tensors'].update(t)
        return loss, features, states, pk['out_state'], pk['metrics'], pk['tensors']


# ---------------------------------------------------------------------------------------------------------------
# actor critic
# ---------------------------------------------------------------------------------------------------------------
class _HeadLoss(torch.autograd.Function):
    """A scalar loss whose gradient w.r.t. one MLP's parameters is produced by dm_mlp_head_bwd."""

    @staticmethod
    def forward(ctx, mlp, pack, *params):
        ctx.mlp, ctx.pack = mlp, pack
        return pack['loss'].clone()

    @staticmethod
    def backward(ctx, grad_loss):
        mlp, pk = ctx.mlp, ctx.pack
        ov = pk.get('overlap')
        if 'pre' in pk:                                   # launched on s_ac inside training_step()
            grads, flat, direct = pk.pop('pre').result()
            fused = getattr(mlp, '_fused', None)
            if fused is None or fused.home is not ov.s_ac or flat is not fused.scratch:
                torch.cuda.current_stream().wait_stream(ov.s_ac)
            else:      # what the backward pass reads was allocated on the caller's stream and is released below: not before s_ac is done with it
                for t in (pk.get('x'), pk.get('acts'), pk.get('dout')):
                    if torch.is_tensor(t):
                        t.record_stream(ov.s_ac)
            # else (Dreamer.pipeline_ac_optimizer): the hand-over, the clip and the AdamW step of this group are enqueued on
            # s_ac behind the backward pass; the caller's stream goes on to the next step's forward without waiting for it
        else:
            grads, flat, direct = mlp.bwd(pk['x'], pk['ldx'], pk['rows'], pk['acts'], pk['dout'], pk['ws'])
        pk.pop('acts', None)
        return (None, None) + _finish_backward(mlp, grads, flat, direct, grad_loss)


class _ProbeLoss(torch.autograd.Function):
    """loss_probe of a probe with one (map), two (goals) or three (map+goals) MLP heads that share ONE probe optimizer: the
    gradients of every head's parameters are produced by dm_mlp_head_bwd from the head's scaled output-gradient rows, inside
    backward() on the caller's stream (the probe reads detached features: nothing else waits for it, and it is small enough
    that pre-launching it on a side stream was not built).  `owner` is the probe (its `_fused` is the probe optimizer), `params`
    are ALL its parameters in parameters() order = the optimizer group's: the gradient buffer is claimed ONCE for that union
    (FusedAdamW.claim_fresh_grads hands out the `.grad` slots only for exactly the group's set) and each head writes its own
    slice, straight into the `.grad` slots when zero_grad() came first, else into a scratch buffer autograd accumulates."""

    @staticmethod
    def forward(ctx, owner, pack, *params):
        ctx.owner, ctx.pack, ctx.params = owner, pack, params
        return pack['loss'].clone()

    @staticmethod
    def backward(ctx, grad_loss):
        owner, pk = ctx.owner, ctx.pack
        if pk.get('consumed'):
            raise RuntimeError('loss_probe.backward() called twice (saved activations were released)')
        plist = list(ctx.params)
        flat, views, direct = _flat_views(plist, grad_loss.device, getattr(owner, '_fused', None))
        gof = {id(p): v for p, v in zip(plist, views)}
        for hp in pk['heads']:
            hp['mlp'].bwd_into(gof, hp['x'], hp['ldx'], hp['rows'], hp['acts'], hp['dout'], hp['ws'])
            for k in ('acts', 'dout', 'x'):
                hp.pop(k, None)
        pk['consumed'] = True
        return (None, None) + _finish_backward(owner, views, flat, direct, grad_loss)


class ActorCritic(_Params):
    """a2c.py:11-152."""

    def __init__(self, in_dim, out_actions, hidden_dim=400, hidden_layers=4, layer_norm=True, gamma=0.999, lambda_gae=0.95,
                 entropy_weight=1e-3, target_interval=100, actor_grad='reinforce', actor_dist='onehot', critic_dist='mse',
                 critic_bins=255, critic_bin_range=20.0, return_norm='none', return_norm_lo=0.05, return_norm_hi=0.95,
                 return_norm_decay=0.99, return_norm_limit=1.0):
        super().__init__()
        if actor_dist not in ACTOR_KINDS or actor_grad != 'reinforce':
            raise NotImplementedError(f'actor_dist={actor_dist!r} / actor_grad={actor_grad!r}: the HIP path builds onehot, '
                                      f'tanh_normal and normal_tanh actors with actor_grad=reinforce (actor_grad=dynamics '
                                      f'asserts in the reference itself, SURVEY 0.5)')
        # the two-hot critic and the percentile return normalisation: refused before anything is allocated
        if critic_dist not in CRITIC_DISTS:
            raise ValueError(f'critic_dist={critic_dist!r}: one of {CRITIC_DISTS}')
        if return_norm not in RETURN_NORMS:
            raise ValueError(f'return_norm={return_norm!r}: one of {RETURN_NORMS}')
        if int(critic_bins) != critic_bins or not 2 <= critic_bins <= 256:
            raise ValueError(f'critic_bins={critic_bins}: 2 .. 256')
        if not (math.isfinite(critic_bin_range) and critic_bin_range > 0):
            raise ValueError(f'critic_bin_range={critic_bin_range}: a finite number > 0')
        if not 0.0 <= return_norm_lo <= return_norm_hi <= 1.0:
            raise ValueError(f'return_norm_lo={return_norm_lo}, return_norm_hi={return_norm_hi}: 0 <= lo <= hi <= 1')
        if not 0.0 <= return_norm_decay < 1.0:
            raise ValueError(f'return_norm_decay={return_norm_decay}: in [0, 1)')
        if not (math.isfinite(return_norm_limit) and return_norm_limit > 0):
            raise ValueError(f'return_norm_limit={return_norm_limit}: a finite number > 0')
        self.dist_kind = ACTOR_KINDS[actor_dist]
        self.in_dim, self.out_actions = in_dim, out_actions
        self.gamma, self.lambda_, self.entropy_weight = gamma, lambda_gae, entropy_weight
        self.target_interval, self.actor_grad, self.actor_dist = target_interval, actor_grad, actor_dist
        self.critic_dist, self.critic_bins, self.critic_bin_range = critic_dist, int(critic_bins), float(critic_bin_range)
        self.return_norm, self.return_norm_q = return_norm, (float(return_norm_lo), float(return_norm_hi))
        self.return_norm_decay, self.return_norm_limit = float(return_norm_decay), float(return_norm_limit)
        actor_out_dim = out_actions if actor_dist == 'onehot' else 2 * out_actions      # a2c.py:35
        critic_out_dim = self.critic_bins if critic_dist == 'twohot' else 1
        self.actor = MLP(in_dim, actor_out_dim, hidden_dim, hidden_layers, layer_norm)
        self.critic = MLP(in_dim, critic_out_dim, hidden_dim, hidden_layers, layer_norm)
        self.critic_target = MLP(in_dim, critic_out_dim, hidden_dim, hidden_layers, layer_norm)
        self.critic_target.requires_grad_(False)
        if critic_dist == 'twohot':
            # a fresh critic gives every bin the same logit: the decoded value of any state is the mean of the symmetric bins, ~0
            out_layer = self.critic.model[3 * hidden_layers]
            nn.init.zeros_(out_layer.weight)
            nn.init.zeros_(out_layer.bias)
            # the symlog-space support, fp32-rounded linspace; not part of state_dict (a function of two config keys)
            self.register_buffer('bins', torch.linspace(-self.critic_bin_range, self.critic_bin_range, self.critic_bins),
                                 persistent=False)
        if return_norm == 'percentile':
            self.register_buffer('return_range', torch.zeros(2))      # the running [lo, hi] percentiles of the imagined returns
        self.train_steps = 0
        self.sparse_cols = 0                  # trailing feature columns known to be one-hot samples (set by the owner)
        self.defer_target_update = False      # a caller that captures the step into a graph does the refresh + counter itself

    def update_critic_target(self):
        """a2c.py:151-152."""
        with torch.no_grad():
            for dst, src in zip(self.critic_target.parameters(), self.critic.parameters()):
                H.call('dm_copy_params', H.fptr(dst), H.fptr(src), dst.numel(), H.stream())

    def begin_step(self, log_only=False):
        """The head of training_step (a2c.py:76-79): refresh the target network every target_interval steps, count the step."""
        if not log_only and not self.defer_target_update:
            if self.train_steps % self.target_interval == 0:
                self.update_critic_target()
            self.train_steps += 1

    @staticmethod
    def split_steps(J):
        """The heads over the (J, M) imagined states run as two row windows, steps [0, split) and [split, J): the first one can
        start while the rollout is still producing the last steps (Dreamer._heads_forward).  Always the same split, so every
        execution order computes the same numbers.  Short horizons: one window."""
        return (J * 5) // 8 if J >= 9 else J

    def value_buffers(self, rows, device):
        bufs = dict(value_t=torch.empty(rows, 1, device=device), value=torch.empty(rows, 1, device=device),
                    c_acts=torch.empty(self.critic.acts_floats(rows), device=device))
        if self.critic_dist == 'twohot':      # the two networks' logit rows, which the scalars above are decoded from
            bufs.update(logits_t=torch.empty(rows, self.critic_bins, device=device),
                        logits=torch.empty(rows, self.critic_bins, device=device))
        return bufs

    def value(self, feats, F_, rows, ws, target=False, window=None, out=None, acts=None, save_acts=False, sparse=True, logits=None):
        """The scalar value of `rows` feature rows - the only place a critic's output becomes a scalar.  target: critic_target
        instead of critic.  window / out / acts / save_acts: as MLP.fwd.  sparse=False: the feature rows' one-hot tail is not
        announced to the first layer (Dreamer.inference / act never did).  Returns (value (rows, 1) - or `out` - , acts).
        critic_dist='mse': exactly that MLP.fwd call.  'twohot': the MLP forward to K logits per row, then dm_twohot_decode
        (symexp of the softmax-weighted mean of the bins); with a window, `logits` is the caller's full (rows_total, K) array."""
        mlp = self.critic_target if target else self.critic
        sp = self.sparse_cols if sparse else 0        # the one-hot latent columns at the end of a feature row (0: unknown)
        if self.critic_dist == 'mse':
            return mlp.fwd(feats, F_, rows, ws, acts=acts, save_acts=save_acts, sparse_cols=sp, window=window, out=out)
        K = self.critic_bins
        if window is not None:
            rows_total, row0 = window
            assert logits is not None and tuple(logits.shape) == (rows_total, K) and out is not None
            mlp.fwd(feats, F_, rows, ws, acts=acts, save_acts=save_acts, sparse_cols=sp, window=window, out=logits)
            lg, v = logits[row0:row0 + rows], out[row0:row0 + rows]
        else:
            lg, acts = mlp.fwd(feats, F_, rows, ws, acts=acts, save_acts=save_acts, sparse_cols=sp)
            out = v = torch.empty(rows, 1, device=lg.device)
        H.call('dm_twohot_decode', rows, K, H.fptr(lg), K, H.fptr(self.bins), H.fptr(v), H.stream())
        return out, acts

    def forward_values(self, feats, F_, rows_total, row0, rows, ws, bufs):
        """critic_target and critic over rows [row0, row0 + rows) of the feature matrix (a2c.py:85,113)."""
        w = (rows_total, row0)
        self.value(feats, F_, rows, ws, target=True, window=w, out=bufs['value_t'], logits=bufs.get('logits_t'))
        self.value(feats, F_, rows, ws, window=w, out=bufs['value'], acts=bufs['c_acts'], save_acts=True, logits=bufs.get('logits'))

    def training_step(self, features, actions, rewards, terminals, log_only=False, act_idx=None, ws=None,
                      actor_acts=None, actor_logits=None, overlap=None, mbuf=None, values=None, _begun=False):
        """features (J,M,F), actions (H,M,A) one-hot, rewards/terminals (J,M). a2c.py:61-149.
        actor_acts / actor_logits: forward_actor(features[:-1]) as already computed by the dream rollout on the same
        features and weights (bit-identical to recomputing it, which is what the reference does, a2c.py:119)."""
        _require_cuda(features, 'features')
        if not _begun:
            self.begin_step(log_only)
        J, M, F_ = features.shape
        Hh, A, dev = J - 1, self.out_actions, features.device
        feats = features.contiguous().view(J * M, F_)
        rewards, terminals = rewards.contiguous(), terminals.contiguous()
        if self.dist_kind == 0:
            if act_idx is None:
                act_idx = actions.argmax(-1).to(torch.int32)
            act_idx = act_idx.contiguous().view(-1)
        if ws is None:
            raise H.DreamerHipError('ActorCritic.training_step needs the model workspace (called through Dreamer.training_step)')

        sp = self.sparse_cols        # the one-hot latent columns at the end of a feature row (0: unknown)
        if values is None:           # (Dreamer.training_step hands them over: computed next to the reward / terminal heads)
            values = self.value_buffers(J * M, dev)
            r0 = self.split_steps(J) * M
            for a, b in ((0, r0), (r0, J * M)):
                if b > a:
                    self.forward_values(feats, F_, J * M, a, b - a, ws, values)
        value_t, value, c_acts = values['value_t'], values['value'], values['c_acts']
        if actor_acts is not None:
            logits, a_acts = actor_logits, actor_acts
        else:
            logits, a_acts = self.actor.fwd(feats, F_, Hh * M, ws, sparse_cols=sp)   # features[:-1] = first H*M rows
        adv, agae, vtgt, wgt = (torch.empty(Hh, M, device=dev) for _ in range(4))
        H.call('dm_gae_losses', Hh, M, self.gamma, self.lambda_, H.fptr(rewards), H.fptr(terminals), H.fptr(value_t),
               H.fptr(adv), H.fptr(agae), H.fptr(vtgt), H.fptr(wgt), H.stream())
        rows = Hh * M
        lc = torch.empty(rows, device=dev)
        gw = float(getattr(self, 'grad_weight', 1.0))          # data-parallel shard weight B_r/B (dist.attach), gradients only
        if self.critic_dist == 'twohot':
            # the two-hot cross-entropy against symlog(value_target); the kernel zeroes the last M rows of the gradient itself
            # (value[-1] gets no gradient) and the loss-only form (log_only) writes none at all
            dvalue = None if log_only else torch.empty(J * M, self.critic_bins, device=dev)
            H.call('dm_twohot_loss', rows, J * M, self.critic_bins, H.fptr(values['logits']), self.critic_bins, H.fptr(self.bins),
                   H.fptr(vtgt), H.fptr(wgt), gw / rows, H.fptr(lc), H.fptr(dvalue), None, H.stream())
        else:
            dvalue = torch.zeros(J * M, 1, device=dev)               # value[-1] gets no gradient
            H.call('dm_critic_loss', rows, H.fptr(value), H.fptr(vtgt), H.fptr(wgt), gw / rows, H.fptr(lc), H.fptr(dvalue),
                   H.stream())
        agae_a = agae            # what the actor loss is scaled by
        if self.return_norm == 'percentile':
            # advantages over max(limit, running percentile range of the imagined returns); the running range moves only on a
            # training step.  No host synchronisation: the scale stays on the device
            agae_a, rn_out = agae.clone(), torch.empty(5, device=dev)
            H.call('dm_return_norm', rows, H.fptr(vtgt), self.return_norm_q[0], self.return_norm_q[1], self.return_norm_decay,
                   self.return_norm_limit, int(torch.is_grad_enabled() and not log_only), H.fptr(self.return_range),
                   H.fptr(rn_out), H.fptr(agae_a), rows, H.stream())
        la, ent = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
        dlogits = torch.empty(rows, self.actor.out_dim, device=dev)
        if self.dist_kind == 0:
            H.call('dm_actor_loss', rows, A, H.fptr(logits), H.ptr(act_idx), H.fptr(agae_a), H.fptr(wgt), self.entropy_weight,
                   gw / rows, H.fptr(la), H.fptr(ent), H.fptr(dlogits), H.stream())
        else:
            H.call('dm_actor_loss_continuous', self.dist_kind, rows, A, H.fptr(logits), H.fptr(actions.contiguous()),
                   H.fptr(agae_a), H.fptr(wgt), self.entropy_weight, gw / rows, H.fptr(la), H.fptr(ent), H.fptr(dlogits),
                   H.stream())
        value2d = value.view(J, M)
        reward1 = rewards.view(J, M)[1:]
        if mbuf is None:
            mbuf = torch.zeros(METRIC_BUF_FLOATS, device=dev)
        s = _multi_sum([(lc, 1.0 / rows), (la, 1.0 / rows), (ent, 1.0 / rows), (value2d[0], 1.0 / M),
                        (value2d[:-1], 1.0 / rows), (reward1, 1.0 / rows)], dev, out=mbuf[8:14])
        std = _multi_sum([(reward1, 1.0 / max(rows - 1, 1), s[5:6], 2)], dev, out=mbuf[14:15])   # unbiased std (a2c.py:140)
        loss_critic_v, loss_actor_v = s[0], s[1]
        if log_only:
            loss_actor, loss_critic = loss_actor_v, loss_critic_v
        else:
            pa = dict(loss=loss_actor_v, x=feats, ldx=F_, rows=rows, acts=a_acts, dout=dlogits, ws=ws, overlap=overlap)
            pc = dict(loss=loss_critic_v, x=feats, ldx=F_, rows=J * M, acts=c_acts, dout=dvalue, ws=ws, overlap=overlap)
            loss_actor = _HeadLoss.apply(self.actor, pa, *self.actor.param_list())
            loss_critic = _HeadLoss.apply(self.critic, pc, *self.critic.param_list())
            self._last_packs = (pa, pc)
        metrics = dict(loss_critic=loss_critic_v, loss_actor=loss_actor_v, policy_entropy=s[2], policy_value=s[3],
                       policy_value_im=s[4], policy_reward=s[5], policy_reward_std=std[0])
        if self.return_norm == 'percentile':
            s0 = RETURN_METRIC_SLOTS['policy_return_lo']
            mbuf[s0:s0 + 3].copy_(rn_out[2:5])
            metrics.update({k: mbuf[i] for k, i in RETURN_METRIC_SLOTS.items()})
        tensors = dict(value=value2d, value_target=vtgt, value_advantage=adv, value_advantage_gae=agae, value_weight=wgt)
        return (loss_actor, loss_critic), metrics, tensors


# ---------------------------------------------------------------------------------------------------------------
# Dreamer
# ---------------------------------------------------------------------------------------------------------------
class Dreamer(nn.Module):
    """dreamer.py:19-226."""

    def __init__(self, conf):
        super().__init__()
        assert conf.action_dim > 0, 'Need to set action_dim to match environment'
        if conf.probe_model not in ('none', 'map', 'goals', 'map+goals'):
            raise NotImplementedError(f'probe_model={conf.probe_model!r}: the probes built are none, map, goals and map+goals')
        if conf.probe_model in ('goals', 'map+goals') and int(getattr(conf, 'goals_size', 0)) < 1:
            raise NotImplementedError(f'probe_model={conf.probe_model!r} needs goals_size >= 1 (got goals_size='
                                      f"{getattr(conf, 'goals_size', 0)}): a zero-width goals decoder is not built in the HIP path")
        if conf.probe_model != 'none' and conf.probe_gradients:
            raise NotImplementedError('probe_gradients=True with a probe model: the gradient of the probe loss into the world '
                                      "model's features is not built (the probe trains on detached features only)")
        if conf.probe_model != 'none' and not dense_image_gate(conf) and imageless_gate(conf):
            raise NotImplementedError(f'probe_model={conf.probe_model!r} on an image-less world model is not built (DESIGN 4.12)')
        features_dim = conf.deter_dim + conf.stoch_dim * (conf.stoch_discrete or 1)
        self.conf = conf
        self.iwae_samples, self.imag_horizon = conf.iwae_samples, conf.imag_horizon
        self.wm = WorldModel(conf)
        self.ac = ActorCritic(in_dim=features_dim, out_actions=conf.action_dim, layer_norm=conf.layer_norm, gamma=conf.gamma,
                              lambda_gae=conf.lambda_gae, entropy_weight=conf.entropy, target_interval=conf.target_interval,
                              actor_grad=conf.actor_grad, actor_dist=conf.actor_dist,
                              **{k: getattr(conf, k) for k in AC_CONF_KEYS if hasattr(conf, k)})
        self.ac.sparse_cols = conf.stoch_dim * conf.stoch_discrete       # feature = [h | one-hot z] (rssm.py:83-84)
        # dreamer.py:43-52: the map probe sees [features | map_coord], the goals probe the bare features
        if conf.probe_model == 'map':
            self.probe_model = MapProbeHead(features_dim + 4, conf)
        elif conf.probe_model == 'goals':
            self.probe_model = GoalsProbe(features_dim, conf)
        elif conf.probe_model == 'map+goals':
            self.probe_model = MapGoalsProbe(features_dim, conf)
        else:
            self.probe_model = NoProbeHead()
        self.probe_gradients = conf.probe_gradients
        self._groups = None
        # conf.amp (defaults.yaml:55; train.py:166 runs the step under autocast): GEMM operands in bf16, fp32 accumulation,
        # fp32 storage.  Precision is an argument of every library call (dm_shape.flags bit DM_FLAG_BF16 via
        # WorldModel.shape(), dm_mlp_params.precision via MLP.struct()); there is no process-wide switch.
        self.amp = bool(getattr(conf, 'amp', False))
        for m in self.modules():
            if isinstance(m, MLP):
                m.precision = int(self.amp)
        self._overlap = None
        self.overlap_backward = True      # pre-launch the three backward passes on side streams (see _Overlap)
        # the world-model forward's tail (decoder, heads, losses) on the world-model stream: WorldModel._forward (A/B: set False)
        self.wm_tail_on_side = True

    # ---- optimizers (dreamer.py:60-87)
    def param_groups(self):
        return dict(wm=list(self.wm.parameters()), probe=list(self.probe_model.parameters()),
                    actor=list(self.ac.actor.parameters()), critic=list(self.ac.critic.parameters()))

    def init_optimizers(self, lr, lr_actor=None, lr_critic=None, eps=1e-5):
        groups = self.param_groups()
        # the auxiliary ActorCritic's actor never receives a gradient (dreamer.py:347-358 keeps only loss_critic): torch's AdamW
        # skips such parameters entirely, so they are frozen here too (its critic_target has requires_grad=False already)
        frozen = list(self.wm.ac_aux.actor.parameters()) if self.wm.ac_aux is not None else []
        self._opt = dict(wm=FusedAdamW(groups['wm'], lr=lr, eps=eps, frozen=frozen), probe=FusedAdamW(groups['probe'], lr=lr, eps=eps),
                         actor=FusedAdamW(groups['actor'], lr=lr_actor or lr, eps=eps),
                         critic=FusedAdamW(groups['critic'], lr=lr_critic or lr, eps=eps))
        # the backward passes write straight into these optimizers' gradient buffers (see _flat_views)
        self.wm._fused, self.ac.actor._fused, self.ac.critic._fused = self._opt['wm'], self._opt['actor'], self._opt['critic']
        if not isinstance(self.probe_model, NoProbeHead):      # _ProbeLoss claims the group's gradient buffer once for all heads
            self.probe_model._fused = self._opt['probe']
        self.prepare_streams()
        if self.probe_gradients:      # dreamer.py:67-71: three optimizers; the probe head's parameters belong to none of them
            return self._opt['wm'], self._opt['actor'], self._opt['critic']
        return self._opt['wm'], self._opt['probe'], self._opt['actor'], self._opt['critic']

    def prepare_streams(self, device=None):
        """Creates the step's side streams and gives each its hardware queue NOW (_Overlap.__init__).  Called by init_optimizers()
        and by dist.attach(model=...); a data-parallel trainer must reach one of them BEFORE its first collective (a barrier and a
        parameter broadcast count): a communicator that exists before these streams have run anything slowed every later step by
        +11 ... +19 ms in round 6's measurement (profiles/r06_force_dp.txt, run J) - the process warns when it sees that order.
        No-op on the CPU, when the streams exist already, and inside a graph capture."""
        if device is None:
            device = next(self.parameters()).device
        device = torch.device(device)
        if device.type != 'cuda' or not self.overlap_backward or torch.cuda.is_current_stream_capturing():
            return
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if self._overlap is None or self._overlap.s_wm.device != device:
            _warn_if_communicator_exists()
            self._overlap = _Overlap(device)

    def grad_clip(self, grad_clip, grad_clip_ac=None):
        if getattr(self, '_opt', None) is None:
            raise RuntimeError('call init_optimizers() before grad_clip(): clipping runs on the optimizers\' flat buffers')
        o = self._opt
        mb = getattr(self, 'metric_buffer', None)
        if mb is not None and mb.device != o['wm'].flat_grad.device:
            mb = None
        if mb is not None and o['actor'].home is not None:
            mb.record_stream(o['actor'].home)      # (pipelined mode: two of its slots are written on the actor-critic stream)
        out = lambda name: None if mb is None else mb[METRIC_SLOTS[name]:METRIC_SLOTS[name] + 2]   # [norm, clip coefficient]
        if self.probe_gradients:      # dreamer.py:81-86
            return dict(grad_norm=o['wm'].clip_grad_norm(grad_clip, out('grad_norm')),
                        grad_norm_actor=o['actor'].clip_grad_norm(grad_clip_ac or grad_clip, out('grad_norm_actor')),
                        grad_norm_critic=o['critic'].clip_grad_norm(grad_clip_ac or grad_clip, out('grad_norm_critic')))
        return dict(grad_norm=o['wm'].clip_grad_norm(grad_clip, out('grad_norm')),
                    grad_norm_probe=o['probe'].clip_grad_norm(grad_clip, out('grad_norm_probe')),
                    grad_norm_actor=o['actor'].clip_grad_norm(grad_clip_ac or grad_clip, out('grad_norm_actor')),
                    grad_norm_critic=o['critic'].clip_grad_norm(grad_clip_ac or grad_clip, out('grad_norm_critic')))

    # ---- pipelined actor / critic optimizer (round 4) --------------------------------------------------------------------
    # The four optimizer groups are independent (dreamer.py:60-71).  With `pipeline_ac_optimizer = True` the gradient hand-over,
    # clip and AdamW step of the ACTOR and CRITIC groups are enqueued on the actor-critic stream, behind their backward pass,
    # instead of on the caller's stream - which therefore no longer waits for the actor-critic backward before the next
    # step's encoder and posterior loop: the tail of step n (actor-critic backward, ~2.5 ms after the world-model backward has
    # finished, profiles/r04_queues_f32.txt) overlaps the head of step n+1.  Same kernels, same per-stream order: bit-identical
    # parameters (test_pipelined_ac_optimizer_is_bit_identical).  The caller's stream waits for those AdamW steps where it
    # first reads actor / critic parameters (the rollout), in inference() and state_dict(), and in packed_metrics() for the two
    # gradient norms.  OFF by default: a trainer that touches actor / critic `.grad`s or reads `grad_norm_actor / _critic` on its
    # own stream between backward() and step() (GradScaler.unscale_ with amp; `.item()` on grad_clip()'s dict) must leave it off
    # or call join_optimizers() first.  bench.py switches it on (its loop reads no per-step scalars).
    pipeline_ac_optimizer = False

    def _set_ac_home(self, ov):
        o = getattr(self, '_opt', None)
        if o is None:
            return
        on = bool(self.pipeline_ac_optimizer) and ov is not None and all(o[k].dp is None for k in ('actor', 'critic')) \
            and not torch.cuda.is_current_stream_capturing()
        for k in ('actor', 'critic'):
            if o[k].home is not None and not on:
                o[k].join()
            o[k].home = ov.s_ac if on else None

    def _ac_pipelined(self):
        o = getattr(self, '_opt', None)
        return o is not None and o['actor'].home is not None

    def _await_ac_optimizers(self):
        """Before the caller's stream first touches what the actor-critic stream may still be using - actor / critic parameters
        (AdamW), the imagined trajectory and the heads' activations of the previous step (its backward pass) - it waits for
        that stream.  By now it holds nothing but the previous step's tail."""
        if self._ac_pipelined():
            self.join_optimizers()

    def join_optimizers(self):
        """The current stream waits for everything the pipelined optimizer groups have enqueued on their own stream."""
        o = getattr(self, '_opt', None)
        if o is not None:
            for k in ('actor', 'critic'):
                o[k].join()

    def state_dict(self, *args, **kwargs):
        self.join_optimizers()
        return super().state_dict(*args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self.join_optimizers()      # (pipelined mode: an actor / critic AdamW step may still be writing the parameters)
        return super().load_state_dict(*args, **kwargs)

    def check_device_status(self):
        """Raises - ONCE - if a persistent posterior kernel of this process has given up in a spin loop (csrc/rssm_lds.hip: it needs
        every workgroup resident at once; a second process on the GPU can starve it).  The flag is host-visible memory the kernel
        writes, so this costs nothing; it is meaningful behind a device synchronisation - packed_metrics_host() and the
        trainer's logging sync are where it is called.  The call ACKNOWLEDGES the flag (dm_rssm_lds_status_ack): the step that
        gave up produced garbage and must not be trusted, so the trainer restores its last checkpoint and goes on IN THIS
        PROCESS - the library keeps the persistent kernel switched off from then on (dm_rssm_lds_gave_up) and every later call
        runs the launch chain, and later logging calls do not raise again."""
        st = H.lib().dm_rssm_lds_status_ack()
        if st != 0:
            raise RuntimeError(f'a persistent RSSM kernel gave up in a spin loop (status {st}): the outputs of that training step '
                               'are invalid - restore the last checkpoint; later steps of this process run the launch chain '
                               '(the persistent kernel stays off) and this error is not raised again')

    def packed_metrics(self):
        """(names, buffer, idx): every loss / metric scalar of the last training_step() (+ the gradient norms once grad_clip()
        has run) sits in ONE 1-D device tensor `buffer`; `idx` (a python list) are the slots of `names` in it, so
        `vals = buffer.tolist(); dict(zip(names, (vals[i] for i in idx)))` replaces the trainer's ~20 `.item()` syncs per
        logged step (train.py:204-214) with a single device-to-host copy.  No kernel runs here: the kernels of the step
        wrote their results straight into this buffer."""
        self.join_optimizers()      # (pipelined mode: the actor / critic gradient norms were written on the actor-critic stream)
        slots = dict(METRIC_SLOTS)
        if isinstance(self.probe_model, (GoalsProbe, MapGoalsProbe)):
            slots.update(GOALS_METRIC_SLOTS)
        if self.ac.return_norm == 'percentile':
            slots.update(RETURN_METRIC_SLOTS)
        if self.wm.kl_free > 0:
            slots.update(KL_FREE_METRIC_SLOTS)
        names = list(slots)
        return names, self.metric_buffer, [slots[n] for n in names]

    def packed_metrics_host(self):
        """{name: float} of packed_metrics() with ONE device-to-host copy (= the step's only sync), followed by
        check_device_status() - the logging call of a trainer (train.py:204-214)."""
        names, buf, idx = self.packed_metrics()
        vals = buf.tolist()
        self.check_device_status()
        return {n: vals[i] for n, i in zip(names, idx)}

    def init_state(self, batch_size):
        return self.wm.init_state(batch_size)

    # ---- inference (dreamer.py:92-111)
    def inference(self, obs, in_state, noise=None):
        """`noise` (beyond the reference signature): dict(u_post (1,B,S)) of explicit uniforms for the posterior draw."""
        assert 'action' in obs, 'Observation should contain previous action'
        act_shape = obs['action'].shape
        assert len(act_shape) == 3 and act_shape[0] == 1, f'Expected shape (1,B,A), got {act_shape}'
        self.join_optimizers()
        features, out_state = self.wm.forward(obs, in_state, None if noise is None else noise['u_post'])
        B = act_shape[1]
        feat = features.reshape(B, -1)
        shp = self.wm.shape(1, B, 1)
        ws = self.wm.workspace(shp, feat.device)
        logits, _ = self.ac.actor.fwd(feat, feat.shape[1], B, ws, save_acts=False)
        value, _ = self.ac.value(feat, feat.shape[1], B, ws, sparse=False)
        action_distr = _torch_actor_distribution(self.ac.actor_dist, logits.view(1, B, -1))
        return action_distr, out_state, dict(policy_value=value.mean())

    # ---- acting (generator.py:311-331 for B environments)
    def act(self, obs, in_state, noise=None, return_rows=False, mode='sample', action_noise=0.0, ac=None):
        """inference() followed, on the device, by what the reference's NetworkPolicy does with the distribution object: the draw,
        log_prob(action).exp().mean(), entropy().mean() and policy_value - one dm_policy_draw call behind the actor and critic MLPs,
        no torch op after them and no host synchronisation.  Returns (action (1,B,A) float32, out_state, metrics): metrics =
        {policy_value, action_prob, policy_entropy}, 0-dim views of ONE 4-float device tensor (reading all three is one copy).
        `obs`, `in_state`: as inference().  `noise`: dict with u_post (1,B,S) as for inference() and / or u_act - (B,) uniforms for
        the one-hot actor, (B,A) standard normals for the continuous ones; what is missing is drawn on the device.  The action is
        the one dm_sample_onehot / dm_sample_continuous give for the actor's output and u_act: the acting and the imagined policy
        are the same function of the same numbers.  tanh_normal's log-probability is taken at the pre-tanh draw, not through atanh
        of the action as the reference's log_prob(action) does (that loses the draw near saturation).
        return_rows=True: metrics also holds log_prob, entropy, value (each (B,)) and, for the one-hot actor, act_idx ((B,) int32).
        mode='mode' (evaluation): the distribution's mode instead of a draw - the lowest argmax class, or the base
        Normal's mean through the transform; u_act is not used.  action_noise > 0 (with mode='sample' only): DreamerV2's exploration
        noise on the drawn action through dm_policy_draw_mode's mode 2 - `noise` may carry u_expl, (B,2) uniforms for the one-hot
        actor or (B,A) standard normals for the continuous ones; log_prob stays the policy's.  The defaults are dm_policy_draw.
        ac: the actor-critic whose actor, critic and distribution kind act (explore.Plan2Explore's exploration policy) behind the
        world model's encoder and posterior step; None: the task one."""
        ac = self.ac if ac is None else ac
        assert 'action' in obs, 'Observation should contain previous action'
        act_shape = obs['action'].shape
        assert len(act_shape) == 3 and act_shape[0] == 1, f'Expected shape (1,B,A), got {act_shape}'
        B, A, kind = act_shape[1], self.conf.action_dim, ac.dist_kind
        noise = noise or {}
        u_act = noise.get('u_act')
        ua_shape = (B,) if kind == 0 else (B, A)
        if u_act is not None and tuple(u_act.shape) != ua_shape:
            raise ValueError(f'actor noise has shape {tuple(u_act.shape)}, expected {ua_shape}')
        if mode not in ('sample', 'mode'):
            raise ValueError(f"mode is {mode!r}, expected 'sample' or 'mode'")
        action_noise = float(action_noise)
        if not action_noise >= 0.0:
            raise ValueError(f'action_noise is {action_noise}, expected a number >= 0')
        if action_noise > 0.0 and mode == 'mode':
            raise ValueError("action_noise > 0 goes with mode='sample': the distribution's mode is taken without noise")
        u_expl = noise.get('u_expl')
        ue_shape = (B, 2) if kind == 0 else (B, A)
        if u_expl is not None and tuple(u_expl.shape) != ue_shape:
            raise ValueError(f'exploration noise has shape {tuple(u_expl.shape)}, expected {ue_shape}')
        draw_mode = 1 if mode == 'mode' else (2 if action_noise > 0.0 else 0)
        with torch.no_grad():
            self.join_optimizers()
            features, out_state = self.wm.forward(obs, in_state, noise.get('u_post'))
            feat = features.reshape(B, -1)
            dev = feat.device
            ws = self.wm.workspace(self.wm.shape(1, B, 1), dev)
            logits, _ = ac.actor.fwd(feat, feat.shape[1], B, ws, save_acts=False)
            value, _ = ac.value(feat, feat.shape[1], B, ws, sparse=False)
            if draw_mode == 1:
                u_act = None
            else:
                if u_act is None:
                    u_act = torch.rand(ua_shape, device=dev) if kind == 0 else torch.randn(ua_shape, device=dev)
                u_act = u_act.float().contiguous()
            if draw_mode == 2:
                if u_expl is None:
                    u_expl = torch.rand(ue_shape, device=dev) if kind == 0 else torch.randn(ue_shape, device=dev)
                u_expl = u_expl.float().contiguous()
            action = torch.empty(1, B, A, device=dev)
            stats = torch.empty(4, device=dev)
            dws = torch.empty(int(H.lib().dm_policy_draw_ws_floats(B)), device=dev)
            rows = torch.empty(2, B, device=dev) if return_rows else None
            act_idx = torch.empty(B, dtype=torch.int32, device=dev) if return_rows and kind == 0 else None
            tail = (H.fptr(value), H.fptr(action), A, H.ptr(act_idx), H.fptr(rows), None if rows is None else H.fptr(rows[1]),
                    H.fptr(stats), H.fptr(dws), dws.numel() * 4, H.stream())
            if draw_mode == 0:
                H.call('dm_policy_draw', kind, B, A, H.fptr(logits), logits.shape[1], H.fptr(u_act), *tail)
            else:
                H.call('dm_policy_draw_mode', kind, draw_mode, action_noise, B, A, H.fptr(logits), logits.shape[1], H.fptr(u_act),
                       H.fptr(u_expl) if draw_mode == 2 else None, *tail)
        metrics = dict(policy_value=stats[0], action_prob=stats[1], policy_entropy=stats[2])
        if return_rows:
            metrics.update(log_prob=rows[0], entropy=rows[1], value=value.view(B))
            if kind == 0:
                metrics['act_idx'] = act_idx
        return action, out_state, metrics

    # ---- imagination (dreamer.py:188-216)
    def dream(self, in_state, imag_horizon, dynamics_gradients=False, u_act=None, u_prior=None, _pack=None):
        if dynamics_gradients:
            raise NotImplementedError('actor_grad=dynamics is not built (and not runnable in the reference, SURVEY 0.5)')
        h, z = in_state
        _require_cuda(h, 'in_state')
        Hh = int(imag_horizon)
        start = torch.cat((h, z), -1).contiguous()           # to_feature (rssm.py:83-84)
        return self._dream_from_features(start, Hh, u_act, u_prior, _pack)

    def _dream_from_features(self, start, Hh, u_act=None, u_prior=None, _pack=None, early=None, ac=None):
        """start: (M,F) rows [h|z] (the world model's feature matrix is passed as is, no concat copy).
        ac: the actor-critic that acts and is evaluated in the dream (explore.Plan2Explore's); None: the task one."""
        c = self.conf
        ac = self.ac if ac is None else ac
        M, dev = start.shape[0], start.device
        F_, A, S = self.wm.features_dim, c.action_dim, c.stoch_dim
        shp = self.wm.shape(1, M, Hh)                        # T*B = M rows for workspace sizing
        ws = self.wm.workspace(shp, dev)
        kind = ac.dist_kind
        # uniforms for the one-hot actor / the categorical latents, standard-normal noise for continuous actors / Gaussian latents
        ua_shape = (Hh, M) if kind == 0 else (Hh, M, A)
        if u_act is not None and tuple(u_act.shape) != ua_shape:
            raise ValueError(f'actor noise has shape {tuple(u_act.shape)}, expected {ua_shape}')
        if u_act is None:
            u_act = torch.rand(ua_shape, device=dev) if kind == 0 else torch.randn(ua_shape, device=dev)
        if u_prior is None:
            u_prior = (torch.rand if c.stoch_discrete else torch.randn)(Hh, M, S, device=dev)
        u_act, u_prior = u_act.float().contiguous(), u_prior.reshape(Hh, M, S).float().contiguous()
        start = start.contiguous()
        feats = torch.empty(Hh + 1, M, F_, device=dev)
        actions = torch.empty(Hh, M, A, device=dev)
        act_idx = torch.empty(Hh, M, dtype=torch.int32, device=dev)
        cell_p = H.rssm_struct(self.wm.core.cell.ordered())
        actor_p = ac.actor.struct()
        a_acts = a_logits = None
        if _pack is not None:          # training: keep the actor activations of all H steps for the policy-gradient backward
            a_acts = torch.empty(int(ac.actor.acts_floats(Hh * M)), device=dev)
            a_logits = torch.empty(Hh * M, ac.actor.out_dim, device=dev)
        # The heads over the imagined states (reward, terminal: dreamer.py:212-213; critic_target, critic: a2c.py:85,113) are
        # per-row work on 40 000 rows, 4 ms behind a rollout whose last steps leave the chip half idle (profiles/r03_queues_*):
        # they run as two row windows - steps [0, split) and [split, H] - and with `early` (the training step's side streams)
        # the first window runs on the idle actor-critic stream as soon as the library reports those rows final, while the
        # rollout finishes on this one.  Same windows, same kernels either way: bit-identical to the single-stream order.
        rows = (Hh + 1) * M
        r_split = ac.split_steps(Hh + 1) * M
        # (not under conf.amp: there the world-model backward chain on the other side stream is the step's critical path and the
        #  early window only takes CUs from it - measured 23.5 vs 23.2 ms; fp32: 37.1 vs 37.3 ms, 7-column shard 11.36 vs 11.50)
        use_early = (early is not None and _pack is not None and r_split < rows and _HEADS_EARLY
                     and not getattr(c, 'amp', False))
        if use_early:
            H.call('dm_dream_rollout_marks', 1, (ctypes.c_int * 1)(r_split // M - 2),
                   (ctypes.c_void_p * 1)(int(early.ev_mark.cuda_event)))
        H.call('dm_dream_rollout', ctypes.byref(shp), M, H.fptr(start), ctypes.byref(cell_p), ctypes.byref(actor_p),
               H.fptr(u_act), H.fptr(u_prior), H.fptr(feats), H.fptr(actions), H.ptr(act_idx),
               H.fptr(a_acts), H.fptr(a_logits), H.ptr(ws), ws.numel(), H.stream())
        f2 = feats.view(rows, F_)
        dec = self.wm.decoder
        outs = dec.dream_buffers(rows, dev)
        values = ac.value_buffers(rows, dev) if _pack is not None else None

        def heads(a, b, wsx):
            if b <= a:
                return
            dec.dream_fwd(f2, a, b - a, wsx, outs)
            if values is not None:
                ac.forward_values(f2, F_, rows, a, b - a, wsx, values)
        if use_early:
            early.s_ac.wait_event(early.ev_mark)
            with torch.cuda.stream(early.s_ac):
                heads(0, r_split, early.ws_ac)
                early.ev_heads.record(early.s_ac)
            heads(r_split, rows, ws)
            torch.cuda.current_stream().wait_event(early.ev_heads)
        else:
            heads(0, r_split, ws)
            heads(r_split, rows, ws)
        term, mu = dec.dream_means(outs)      # the mean-only form of either head, one launch over all rows behind the windows
        if _pack is not None:
            _pack.update(act_idx=act_idx, ws=ws, actor_acts=a_acts, actor_logits=a_logits, values=values, head_outs=outs)
        return feats, actions, _Mean(mu.view(Hh + 1, M)), _Mean(term.view(Hh + 1, M))

    # ---- training step (dreamer.py:113-186)
    def training_step(self, obs, in_state, iwae_samples=None, imag_horizon=None, do_open_loop=False, do_image_pred=False,
                      do_dream_tensors=False, noise=None, forced_idx=None):
        """Extra keyword arguments beyond the reference signature: `noise` = dict(u_post (T,B,S), u_act (H,M), u_prior
        (H,M,S)) of explicit uniforms for the three sampler call sites, `forced_idx` (T,B,S) to teacher-force the posterior."""
        for k in ('action', 'reward', 'reset', 'terminal'):
            assert k in obs, f'`{k}` required in observation'
        iwae_samples = int(iwae_samples or self.iwae_samples)
        imag_horizon = int(imag_horizon or self.imag_horizon)
        if self.wm.dense and iwae_samples > 1:      # before anything is allocated or launched
            raise NotImplementedError('iwae_samples > 1 is not built on the dense image path (DESIGN 4.11)')
        if self.wm.kl_free > 0 and iwae_samples > 1:
            raise NotImplementedError('kl_free > 0 with iwae_samples > 1: the sampled KL has no per-row exact KL to clip')
        T, B = obs['action'].shape[:2]
        noise = noise or {}
        I = iwae_samples
        u_post = noise.get('u_post')
        if u_post is not None:
            u_post = u_post.reshape(T, B * I, -1)

        if self._overlap is not None:
            # pre-launched backward passes of a step whose losses were never backpropagated may still be using the side streams' workspaces -
            # and their launcher jobs may still be ENQUEUING: a stream wait only orders what is already in the stream, so the
            # jobs are awaited first (their exceptions belong to the backward() that owns them, not to this step)
            stale = [getattr(self.wm, '_last_pack', None)] + list(getattr(self.ac, '_last_packs', None) or ())
            for old_pk in stale:
                fut = old_pk.get('pre') if isinstance(old_pk, dict) else None
                if fut is not None:
                    try:
                        fut.result()
                    except Exception:
                        pass
            cur = torch.cuda.current_stream()
            cur.wait_stream(self._overlap.s_wm)
            if not self._ac_pipelined():          # (pipelined mode waits for the actor-critic stream where the rollout starts:
                cur.wait_stream(self._overlap.s_ac)      # nothing the world-model forward writes is read by that stream)
        # every loss / metric scalar of this step lands in ONE device buffer (METRIC_SLOTS)
        mbuf = torch.zeros(METRIC_BUF_FLOATS, device=obs['action'].device)
        self.metric_buffer = mbuf
        tail = None
        dev0 = obs['action'].device
        if (self.overlap_backward and torch.is_grad_enabled() and self.wm_tail_on_side and dev0.type == 'cuda'
                and not torch.cuda.is_current_stream_capturing()):
            if self._overlap is None or self._overlap.s_wm.device != dev0:
                self._overlap = _Overlap(dev0)
            tail = self._overlap
        loss_model, features, states, out_state, metrics, tensors = \
            self.wm.training_step(obs, in_state, iwae_samples=iwae_samples, do_open_loop=do_open_loop,
                                  do_image_pred=do_image_pred, u_post=u_post, forced_idx=forced_idx,
                                  imag_horizon=imag_horizon, u_pred=noise.get('u_pred'), mbuf=mbuf, _tail=tail)
        pk = self.wm._last_pack
        ov = None
        if not (self.overlap_backward and torch.is_grad_enabled()):
            self._set_ac_home(None)
        if self.overlap_backward and torch.is_grad_enabled():
            dev = pk['feat'].device
            if self._overlap is None or self._overlap.s_wm.device != dev:
                self._overlap = _Overlap(dev)
            ov = self._overlap
            pk['overlap'] = ov
            self._set_ac_home(ov)
            gens = {}
            for owner in (self.wm, self.ac.actor, self.ac.critic):      # main thread: zero_grad() - or a backward() on
                if getattr(owner, '_fused', None) is not None:          # an OLDER step's losses - may come before the
                    gens[id(owner)] = owner._fused.claim_scratch()      # launcher thread has touched the buffers
            # world-model backward: on its own stream and workspace, concurrent with everything below
            ov.ws_wm = _grow_ws(ov.ws_wm, pk['ws'].numel(), dev)
            # (with the forward's tail already on s_wm the backward simply follows it in stream order)
            ov.ev_wm_fwd.record(ov.s_wm if pk.get('tail') is not None else torch.cuda.current_stream())
            pk['pre'] = ov.submit(ov.s_wm, ov.ev_wm_fwd, lambda: self.wm._backward(
                pk, ov.ws_wm, scratch=gens.get(id(self.wm), True), defer_wgrad=True))
        metrics, tensors = dict(metrics), tensors.copy()          # LazyTensors.copy(): image_rec stays a thunk
        if not isinstance(self.probe_model, NoProbeHead):      # the probe's scalars land in the step's metric buffer
            loss_probe, metrics_probe, tensors_probe = self.probe_model.training_step(features.detach(), obs, mbuf=mbuf)
        else:
            loss_probe, metrics_probe, tensors_probe = self.probe_model.training_step(features.detach(), obs)
        metrics.update(**metrics_probe)
        tensors.update(**tensors_probe)

        # (T,B,I) => (TBI): the feature matrix [h|z] of all posterior states, detached (dreamer.py:149)
        dpk = {}
        if ov is not None:
            need = 4 * int(H.lib().dm_mlp_ws_floats((imag_horizon + 1) * T * B * I, MLP_HIDDEN, 4))
            ov.ws_ac = _grow_ws(ov.ws_ac, need, pk['feat'].device)
        self._await_ac_optimizers()      # (pipelined mode: the previous step's actor / critic AdamW ran on the actor-critic stream)
        self.ac.begin_step()             # the target-network refresh comes before the first use of critic_target (a2c.py:76-79)
        features_dream, actions_dream, rewards_dream, terminals_dream = \
            self._dream_from_features(pk['feat'], imag_horizon,
                                      noise.get('u_act') if self.ac.dist_kind == 0 else noise.get('eps_act'),
                                      noise.get('u_prior'), _pack=dpk, early=ov)
        (loss_actor, loss_critic), metrics_ac, tensors_ac = \
            self.ac.training_step(features_dream, actions_dream, rewards_dream.mean, terminals_dream.mean,
                                  act_idx=dpk['act_idx'], ws=dpk['ws'], actor_acts=dpk['actor_acts'],
                                  actor_logits=dpk['actor_logits'], overlap=ov, mbuf=mbuf, values=dpk['values'], _begun=True)
        if ov is not None:
            ov.ev_fwd.record(torch.cuda.current_stream())
            for mlp, hp in zip((self.ac.actor, self.ac.critic), self.ac._last_packs):
                hp['pre'] = ov.submit(ov.s_ac, ov.ev_fwd, lambda mlp=mlp, hp=hp: mlp.bwd(
                    hp['x'], hp['ldx'], hp['rows'], hp['acts'], hp['dout'], ov.ws_ac, scratch=gens.get(id(mlp), True)))
        metrics.update(**metrics_ac)
        if I == 1:
            tensors.update(policy_value=tensors_ac['value'][0].view(T, B))
        else:                        # unflatten_batch(value[0], (T,B,I)).mean(-1), dreamer.py:159
            tensors.update(policy_value=_reduce_i(tensors_ac['value'][0].contiguous().view(-1), T * B, I, 0).view(T, B))
        # Diagnostics for tests / debugging (not part of the reference API).  The index tensors are copies; `actions`,
        # `dream_features`, `post` and `prior` are the step's own buffers.  dream_reward / dream_terminal: the two heads' decoded
        # means over the imagined states, (H + 1, M), as the actor-critic reads them; dream_reward_out: the reward head's own output
        # rows behind them ((H + 1) M, out_dim) - the logits of a two-hot or categorical head, the mean itself for the Normal head.
        self.last_extras = dict(post_idx=pk['idx'].view(T, B * I, -1).clone(), act_idx=dpk['act_idx'].clone(),
                                actions=actions_dream, dream_features=features_dream, actor_logits=dpk.get('actor_logits'),
                                ac_tensors=tensors_ac, post=pk['post'], prior=pk['prior'], pred_idx=pk.get('pred_idx'),
                                dream_reward=rewards_dream.mean, dream_terminal=terminals_dream.mean,
                                dream_reward_out=dpk['head_outs'][0])
        # Dream for a log sample (dreamer.py:163-180): T-1 imagined steps from the B first states, decoded to images
        dream_tensors = {}
        if do_dream_tensors and not self.wm.imageless:      # dreamer.py:164: skipped when there is no image decoder
            with torch.no_grad():
                kind, dpk2 = self.ac.dist_kind, {}
                # states[0, :, 0] (dreamer.py:170): the first of the I samples of every batch column at t = 0 = rows b*I
                f2, a2, r2, t2 = self._dream_from_features(
                    pk['feat'][:B * I:I].contiguous(), T - 1,
                    noise.get('u_act_log') if kind == 0 else noise.get('eps_act_log'), noise.get('u_prior_log'), _pack=dpk2)
                shp = pk['shp_e']          # (T,B,1): the log dream has one row per (step, column)
                ws = self.wm.workspace(shp, pk['feat'].device)
                # decoder.image.forward (dreamer.py:171); on the dense path the raw logits, not normalised
                _, image_dream = self.wm.decoder.decode(shp, f2.view(T * B, -1), pk['image'], ws, raw=True)
                _, _, t_ac2 = self.ac.training_step(f2, a2, r2.mean, t2.mean, log_only=True, act_idx=dpk2['act_idx'],
                                                    ws=dpk2['ws'], actor_acts=dpk2['actor_acts'],
                                                    actor_logits=dpk2['actor_logits'], values=dpk2['values'])
                dream_tensors = dict(action_pred=torch.cat([obs['action'][:1].float(), a2]), reward_pred=r2.mean,
                                     terminal_pred=t2.mean, image_pred=image_dream.view(T, B, *image_dream.shape[-3:]),
                                     **t_ac2)
                self.last_extras.update(dream_log_act_idx=dpk2['act_idx'].clone(), dream_log_reward_out=dpk2['head_outs'][0])
        if pk.get('tail') is not None:      # losses, metrics and tensors of the world model were written on the world-model stream
            cur = torch.cuda.current_stream()
            cur.wait_event(pk['tail'].ev_tail)
            # ... and ALLOCATED from that stream's pool: what leaves training_step() is read on the caller's stream from here on, so the
            # caching allocator must not hand such a block to the next s_wm allocation while a caller-stream read is still queued
            # (the actor-critic outputs are guarded the same way)
            leaving = [loss_model, pk.get('dec_acts'), pk.get('dec_logits'), pk.get('target'), pk.get('closed')] + [v for v in dict.values(pk['tensors']) if torch.is_tensor(v)]
            for t in leaving:
                if torch.is_tensor(t) and t.is_cuda:
                    t.record_stream(cur)
        if self.probe_gradients:      # dreamer.py:183-186
            losses = (loss_model + loss_probe, loss_actor, loss_critic)
        else:
            losses = (loss_model, loss_probe, loss_actor, loss_critic)
        return losses, out_state, metrics, tensors, dream_tensors

    def __str__(self):
        count = lambda m: sum(p.numel() for p in m.parameters())
        s = [f'Model: {count(self)} parameters']
        for sub in (self.wm.encoder, self.wm.decoder, self.wm.core, self.ac, self.probe_model):
            s.append(f'  {type(sub).__name__:<15}: {count(sub)} parameters')
        return '\n'.join(s)



def __getattr__(name):
    """`from pydreamer_amd.models import WorldModelProbe` (train.py:104-107 picks Dreamer or WorldModelProbe from one module): the
    class lives in baselines.py, which imports this module, so it is looked up on first use instead of imported here."""
    if name == 'WorldModelProbe':
        from .baselines import WorldModelProbe
        return WorldModelProbe
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
