"""-m gpu: integer class-map frames through both device feeds (image_categorical = C; the `minigrid` section).

The repository of tests/class_image_repo.py in tmp_path with S in {7, 8}: a 49-byte image row takes dm_replay_gather's byte lanes, a
64-byte row its 16-byte lanes.  Every feed comparison is exact equality of bytes.
  1. DeviceReplay and DeviceRing(ReplayFeed) hand over batches equal to each other and to preprocess_batch (`image` = the argmax of
     its one-hot), three batches that hold an artificial reset mark and a two-piece column and then past the depth=3 slots' reuse;
     once without a capacity and once with capacity_bytes small enough to evict a file and upload it again.
  2. One Dreamer step and one WorldModelProbe(model='gru_probe') step at the tiny minigrid conf with closed-form weights give the
     same bits on DeviceReplay's batch (uint8 class image, integer map) as on preprocess_batch's (float one-hots): loss, every
     gradient, tensors."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import class_image_repo as CR                        # noqa: E402
import closed_form_params as CFP                     # noqa: E402
from oracle import dreamer_oracle as O               # noqa: E402
from pydreamer_amd import config                     # noqa: E402
from pydreamer_amd import replay as R                # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NB = 6          # batches drawn: the three compared first, then the three depth=3 slots a second time


def _replay(repo):
    return R.SequentialReplay(repo, seed=CR.SEED, **CR.READER)


def _device_replay(repo, evict):
    probe = R.DeviceReplay(_replay(repo), CR.ACTIONS, **CR.FEED)
    sizes = []
    for _ in range(NB):
        sizes += [e.nbytes for e in probe.plan().entries()]
    dr = R.DeviceReplay(_replay(repo), CR.ACTIONS, DEV, depth=3, capacity_bytes=int(1.5 * max(sizes)) if evict else 0, **CR.FEED)
    prepared, prepare = [], dr._prepare
    dr._prepare = lambda info: (prepared.append(info.path), prepare(info))[1]
    return dr, prepared


@pytest.mark.parametrize('evict', [False, True])
@pytest.mark.parametrize('S', [7, 8])
def test_both_device_feeds_equal_preprocess_batch(hip, tmp_path, S, evict):
    repo = CR.write(tmp_path, S)
    dr, prepared = _device_replay(repo, evict)
    ring = R.DeviceRing(R.ReplayFeed(_replay(repo), CR.ACTIONS, **CR.FEED), DEV, depth=3)
    assert dr.spec() == ring.feed.spec() and dr.row_bytes['image'] == S * S
    assert dr.spec()['image'] == ((CR.T, CR.B, S, S), np.uint8)
    handed = []
    for i in range(NB):
        a, b = dr.next(), ring.next()
        if i % 2:
            dr.prefetch(), ring.prefetch()                     # staged ahead, while the handed batch is still being read
        assert all(v.is_cuda for v in a.values()) and all(v.is_cuda for v in b.values())
        handed.append(({k: v.clone() for k, v in a.items()}, {k: v.clone() for k, v in b.items()}))
    torch.cuda.synchronize()
    dr.close(), ring.close()
    # under the small capacity a file was dropped, chosen again, read and uploaded again; without one every file is prepared once
    assert (len(prepared) > len(set(prepared))) == evict and (len(dr._cache) < len(dr.replay.files)) == evict
    assert all(h is not None for h in dr._held), 'every device slot was gathered into (and reused)'
    two_piece = marked = False
    plans = R.DeviceReplay(_replay(repo), CR.ACTIONS, **CR.FEED)
    for i, ((a, b), (want, onehot, _)) in enumerate(zip(handed, CR.reference_batches(repo, NB))):
        if i < 3:
            plan = plans.plan()
            two_piece |= bool((plan.pieces[:, 1, 1] > 0).any())
            marked |= bool(plan.pieces[:, :, 2].any())
        for who, got in (('DeviceReplay', a), ('DeviceRing', b)):
            got = {k: v.cpu().numpy() for k, v in got.items()}
            CR.same(got, want, (who, S, evict, i))
            assert np.array_equal(got['image'], onehot.argmax(2))
    assert two_piece and marked, 'the first three batches must hold a two-piece column and an artificial reset mark'


def _conf(S, **more):
    tiny = dict(deter_dim=64, hidden_dim=64, stoch_dim=8, stoch_discrete=8, batch_length=CR.T, batch_size=CR.B, imag_horizon=4,
                image_size=S, image_channels=CR.CLASSES, action_dim=CR.ACTIONS, map_size=CR.MAP_SIZE, map_channels=CR.MAP_CLASSES,
                map_hidden_dim=128, map_hidden_layers=2, probe_model='map')
    return config.load_config('defaults', 'minigrid', **{**tiny, **more})


def _step(conf, cls, obs, noise):
    """One trainer iteration of a fresh model with closed-form weights: (losses, flat gradients, tensors)."""
    model = cls(conf)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(CFP.make_params(shapes, seed=0), strict=True)
    model = model.to(DEV)
    opts = model.init_optimizers(conf.adam_lr, conf.adam_lr_actor, conf.adam_lr_critic, conf.adam_eps)
    kw = {} if noise is None else dict(noise=noise)
    losses, _, metrics, tensors, _ = model.training_step(obs, model.init_state(conf.batch_size), **kw)
    for opt in opts:
        opt.zero_grad()
    for loss in losses:
        loss.backward()
    model.grad_clip(conf.grad_clip, conf.grad_clip_ac)
    torch.cuda.synchronize()
    return [float(l.detach()) for l in losses],[o.flat_grad.clone() for o in opts], {k: v.clone() for k, v in tensors.items()}


@pytest.mark.parametrize('S', [7, 8])
def test_model_steps_on_the_feed_batch_equal_those_on_preprocess_batch(hip, tmp_path, S):
    from pydreamer_amd.models import Dreamer, WorldModelProbe
    repo = CR.write(tmp_path, S)
    dr = R.DeviceReplay(_replay(repo), CR.ACTIONS, DEV, **CR.FEED)
    for _ in range(3):          # the third batch: carried cursors, past the first files' random starts
        fed = dr.next()
    fed = {k: v.clone() for k, v in fed.items()}
    dr.close()
    want, onehot, map_onehot = CR.reference_batches(repo, 3)[2]
    assert fed['image'].dtype == torch.uint8 and tuple(fed['image'].shape) == (CR.T, CR.B, S, S)
    assert np.array_equal(fed['image'].cpu().numpy(), want['image'])
    host = {k: torch.from_numpy(v).to(DEV) for k, v in dict(want, image=onehot, map=map_onehot).items()}
    assert host['image'].is_floating_point() and host['image'].dim() == 5 and host['map'].dim() == 5
    for cls, more in ((Dreamer, {}), (WorldModelProbe, dict(model='gru_probe', probe_gradients=True))):
        conf = _conf(S, **more)
        noise = None
        if cls is Dreamer:
            oconf = O.make_conf(**{k: getattr(conf, k) for k in O.DEFAULTS})
            noise = {k: v.to(DEV) for k, v in O.make_noise(oconf, seed=5).items() if k in ('u_post', 'u_act', 'u_prior')}
        la, ga, ta = _step(conf, cls, fed, noise)
        lb, gb, tb = _step(conf, cls, host, noise)
        assert la == lb and all(np.isfinite(la)), (cls.__name__, la, lb)
        assert len(ga) == len(gb) and all(torch.equal(x, y) for x, y in zip(ga, gb)), f'{cls.__name__}: gradients differ'
        assert sum(float(x.abs().sum()) for x in ga) > 0
        assert list(ta) == list(tb)
        for k in ta:
            x, y = (torch.nan_to_num(t, nan=-1.0) if t.is_floating_point() else t for t in (ta[k], tb[k]))
            assert torch.equal(x, y), (cls.__name__, k)
