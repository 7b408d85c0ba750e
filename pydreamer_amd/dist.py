"""Data parallelism over the batch axis: one process per GPU, RCCL all-reduce of each optimizer group's flat gradient
buffer over xGMI (torch.distributed backend "nccl" IS RCCL on ROCm).  The reference has no data parallelism at all
(SURVEY.md 2.2); this keeps single-GPU semantics: every rank steps identical replicated AdamW state.

Sharding rule: rank r takes columns B_r of every (T,B,...) tensor; B need not divide evenly
(B=50 over 8 ranks -> 7,7,6,6,6,6,6,6).  A rank's losses are means over ITS T*B_r rows, so its gradients are weighted
by B_r/B before the SUM all-reduce; the result equals the single-process gradient of the global-batch mean.

Every group is reduced late, inside grad_clip() (FusedAdamW.clip_grad_norm), from the main thread in optimizer order, so
every rank issues its collectives in the same order.  The launcher thread (models._Overlap) needs no ordering against them:
the pre-launched backward passes write only the `scratch` buffer, and each collective reads `flat_grad` after
loss.backward() has joined that group's launcher job and handed the buffer over (models._finish_backward ->
FusedAdamW.adopt_scratch).  Over a one-rank RCCL group this costs +0.03 ... +0.06 ms per step (bench.py --force-dp,
profiles/r06_force_dp.txt); the early, overlapped forms round 6 measured were slower and are gone.
"""
import torch
import torch.distributed as dist


def shard_bounds(batch, world, rank):
    """[lo, hi) columns of the global batch owned by `rank` (first `batch % world` ranks get one extra)."""
    base, extra = divmod(batch, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def shard_obs(obs, world, rank):
    """Slice a time-major observation dict on the batch axis (dim 1)."""
    B = obs['action'].shape[1]
    lo, hi = shard_bounds(B, world, rank)
    return {k: v[:, lo:hi].contiguous() for k, v in obs.items()}, (lo, hi)


def attach(optimizers, local_batch, global_batch, group=None, model=None, force=False):
    """Enable gradient all-reduce inside FusedAdamW.clip_grad_norm for every optimizer group.
    model (a pydreamer_amd Dreamer whose init_optimizers() produced `optimizers`): the B_r/B weight is FOLDED into the scale
    argument every backward entry point already takes (models.WorldModel / ActorCritic.grad_weight), so the rank's gradient
    buffers come out of the backward kernels already weighted and no extra pass over the 92 MB buffer runs per step; without
    it (or for a group fed by autograd, the 1-element group of probe_model='none') the buffer is multiplied before the collective."""
    if not dist.is_initialized() or (dist.get_world_size(group) == 1 and not force):
        return      # (force: a ONE-rank group still issues its collectives - bench.py --force-dp measures their cost on a 1-GPU box)
    ac = getattr(model, 'ac', None)
    if getattr(ac, 'return_norm', 'none') == 'percentile' and dist.get_world_size(group) > 1:
        raise NotImplementedError("return_norm='percentile' with a data-parallel group of more than one rank: every rank would "
                                  'normalise by the percentiles of its own shard (reducing them across ranks is not built)')
    w = float(local_batch) / float(global_batch)
    folded = set()
    if model is not None and hasattr(model, 'prepare_streams'):
        model.prepare_streams()      # the step's streams take their hardware queues before any communicator is built (models.Dreamer.prepare_streams)
    if model is not None and getattr(model, '_opt', None) is not None:
        model.wm.grad_weight = w
        model.ac.grad_weight = w
        folded = {id(model._opt[k]) for k in ('wm', 'actor', 'critic')}
        if not hasattr(model.probe_model, 'dummy'):      # every probe but NoProbeHead scales its own gradient rows
            # (models.MapProbeHead, GoalsProbe; MapGoalsProbe hands the weight to both of its heads)
            model.probe_model.grad_weight = w
            folded.add(id(model._opt['probe']))
    for opt in optimizers:
        opt.dp = (group, w)
        opt.dp_folded = id(opt) in folded


def _weight(opt, buf):
    group, w = opt.dp
    if w != 1.0 and not getattr(opt, 'dp_folded', False):
        buf.mul_(w)
    return group


def allreduce_grads(opt):
    """grad <- sum_r (B_r/B) grad_r, in place on the flat buffer (one collective per optimizer group)."""
    group = _weight(opt, opt.flat_grad)
    dist.all_reduce(opt.flat_grad, op=dist.ReduceOp.SUM, group=group)
