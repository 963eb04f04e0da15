"""Env-parallel sharding over the GPUs of one node (one process per GPU, torch.distributed; backend
"nccl" is RCCL over xGMI on ROCm). Environments are fully independent, so the data
path has NO collective: each rank simulates its own shard; the only exchange is one all-gather of
the fixed-size metrics vector per reporting interval."""
import torch
import torch.distributed as dist

from . import _capi


def shard_range(n_total, rank, world):
    """Contiguous shard [lo, hi) of n_total envs for `rank` (sizes differ by at most one)."""
    base, rem = divmod(int(n_total), int(world))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def set_shard_exploration(batch, sigma, seed, n_total, rank, world):
    """Exploration noise (BatchedIntersections.set_exploration) for the shard `rank` holds of n_total environments: its
    env_offset is the shard's first global env index, so the ranks together draw what one batch of n_total envs draws."""
    batch.set_exploration(sigma, seed, env_offset=shard_range(n_total, rank, world)[0])


def generate_shard_arrivals(batch, rate, n_total, rank, world, horizon_s=None, rows=None, seed=0, epoch=0, min_gap=1.0, covered=False):
    """Arrival streams (BatchedIntersections.generate_arrivals) for the shard `rank` holds of n_total environments: its
    env_offset is the shard's first global env index, so the ranks together generate what one batch of n_total envs generates.
    rate: a scalar, or [n_total] (every rank passes the whole vector: the shard's piece is cut here and the row count follows
    the largest rate of all, so every rank allots the same rows)."""
    import numpy as np
    from .arrivals import default_rows
    lo, hi = shard_range(n_total, rank, world)
    r = np.asarray(rate.cpu().numpy() if torch.is_tensor(rate) else rate, np.float64)
    if rows is None and horizon_s is not None:
        rows = default_rows(r, horizon_s)
    return batch.generate_arrivals(r[lo:hi] if r.ndim else float(r), horizon_s=horizon_s, rows=rows, seed=seed, epoch=epoch, env_offset=lo,
                                   min_gap=min_gap, covered=covered)


def metrics_vector(metrics, device, extra=()):
    return torch.tensor([metrics[k] for k in _capi.METRIC_NAMES] + [float(x) for x in extra], dtype=torch.float64,
                        device=device)


def gather_metrics(metrics, device=None, extra=()):
    """All-gather each rank's metrics dict (12 x f64 = 96 B per rank) and return
    (per_rank [world, 12 + len(extra)] tensor on CPU, global dict of sums). `extra`: a few more per-rank numbers
    that ride in the same vector (e.g. the rank's own wall-clock), so that reporting stays ONE collective.
    Works without an initialised process group (world = 1)."""
    if not (dist.is_available() and dist.is_initialized()):
        v = metrics_vector(metrics, "cpu", extra)
        return v[None, :], dict(metrics)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else "cpu"
    v = metrics_vector(metrics, device, extra)
    out = [torch.empty_like(v) for _ in range(dist.get_world_size())]
    dist.all_gather(out, v)
    per_rank = torch.stack(out).cpu()
    tot = per_rank.sum(0)
    return per_rank, {k: float(tot[i]) for i, k in enumerate(_capi.METRIC_NAMES)}
