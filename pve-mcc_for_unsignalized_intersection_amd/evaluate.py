"""`python -m pve_mcc_amd.evaluate --mat data/test/arvTimeNewVeh_new_1000_12.mat --weights actor.npz`

The evaluation protocol of the reference's `main.py:test()` / `batch_test()` (main.py:367-441, 530-584) run
entirely on the GPU: the pretrained MADDPG actor (on-device inference) closes the loop around the fused tick, and
the aggregate lines of main.py:523-526 / 576-581 are printed from the metrics vector:

    vehicle number, collisions occurred number, collisions rate, pT-m (mean passing time), mean jerk, lock_num

One arrival stream can be replicated over many environments (`--envs`, independent copies are identical) or a
synthetic batch can be evaluated (`--synthetic RATE`).

`--rates 1200,1000,900,800,600,400,200` is batch_test()'s sweep over densities (main.py:543-583) as ONE batch: every density
gets `--envs` environments whose arrival streams are generated on the device at its rate, the environments are grouped by
density, and one line per density is printed in batch_test()'s wording from the grouped metrics and roll-out statistics
(metrics_by_group / rollout_stats), read back once at the end."""
import argparse
import json

import numpy as np

from .arrivals import load_arrival_mat, pad_stream, synthetic_arrivals, synthetic_intentions
from ._capi import METRIC_NAMES as _METRIC_NAMES
from .batched import BatchedIntersections


def evaluate(arrivals, weights, ticks=1000, n_envs=1, capacity=128, device="cuda", intentions=None, **config):
    """-> dict with the quantities main.py prints at the end of test() (main.py:523-526).
    config: reference constructor arguments (vm, lane_num = 12 | 8 | 4, ...; main.py --lane_num, :101)."""
    env = BatchedIntersections(n_envs, capacity, arrivals, device=device, intentions=intentions,
                               outputs=("obs_post", "reward", "flags", "env_out"), **config)
    env.set_actor(weights)
    env.reset()
    for _ in range(ticks):
        env.step_with_actor()
    m = env.metrics()
    dt = float(env.cfg.deltaT)
    return {
        "vehicles": m["spawned"], "passed": m["passed"], "collisions": m["collided"],
        "collisions_rate": m["collided"] / max(m["spawned"], 1.0),
        "pT_m": m["passed_steps"] / (m["passed"] + 1e-4) * dt,            # main.py:526
        "jerk_mean": m["sum_jerk"] / max(m["passed"], 1.0),                # main.py:524
        "lock_num": m["locks"], "reward_mean": m["sum_reward"] / max(m["ctl_steps"], 1.0),
        "ticks": ticks, "n_envs": n_envs, "overflow": m["overflow"],
    }


def evaluate_rates(rates, weights, ticks=1000, envs_per_rate=1, capacity=128, device="cuda", seed=20250213, epoch=0, chunk=50,
                   **config):
    """batch_test() (main.py:543-583) over several densities in one batch: len(rates) x envs_per_rate environments, the
    arrival stream of each generated on the device at its rate (generate_arrivals), grouped by rate.  The closed loop runs
    in calls of `chunk` ticks into one reused trajectory buffer; after every call rollout_stats adds the call's ticks to the
    per-rate totals on the device; metrics_by_group reads the headers at the end.  One read-back, after the last tick.
    -> list of one dict per rate (the order of `rates`) with the quantities of main.py:576-581 and the reward mean / standard
    deviation over controlled vehicles (main.py:573-574 prints them for one tick; here they cover the run)."""
    import torch
    from . import stats
    rates = [float(r) for r in rates]
    R, n = len(rates), int(envs_per_rate)
    env = BatchedIntersections(R * n, capacity, None, device=device, outputs=("obs_post", "obs_pre", "reward", "flags", "env_out"),
                               **config)
    dt = float(env.cfg.deltaT)
    env.generate_arrivals(np.repeat(np.asarray(rates), n), horizon_s=ticks * dt + 30.0, seed=seed, epoch=epoch)
    groups = torch.as_tensor(np.repeat(np.arange(R, dtype=np.int32), n)).to(env.device)
    env.set_actor(weights)
    env.reset()
    ring = env.alloc_trajectory(min(chunk, ticks))
    totals = torch.zeros(R, stats.STAT_N, dtype=torch.float64, device=env.device)
    done = 0
    while done < ticks:
        k = min(chunk, ticks - done)
        env.step_many(k, source="actor", trajectory=ring)
        env.rollout_stats(groups=groups, n_groups=R, totals=totals)
        done += k
    m = env.metrics_by_group(groups, R).cpu().numpy()                       # the one read-back (waits for the stream)
    s = stats.summaries(totals)
    col = {name: k for k, name in enumerate(_METRIC_NAMES)}
    out = []
    for g, rate in enumerate(rates):
        spawned, passed, collided = m[g, col["spawned"]], m[g, col["passed"]], m[g, col["collided"]]
        out.append({"rate": rate, "vehicles": spawned, "passed": passed, "collisions": collided,
                    "collisions_rate": collided / max(spawned, 1.0),
                    "pT_m": m[g, col["passed_steps"]] / (passed + 1e-4) * dt,            # main.py:579
                    "jerk_mean": m[g, col["sum_jerk"]] / max(passed, 1.0),                # main.py:580
                    "lock_num": m[g, col["locks"]], "reward_mean": float(s["reward_mean"][g]), "reward_std": float(s["reward_std"][g]),
                    "v_mean": float(s["v_mean"][g]),
                    "ticks": ticks, "n_envs": n, "overflow": m[g, col["overflow"]]})
    return out


def rate_line(res):
    """One density's result in the wording of batch_test() (main.py:576-581)"""
    return "vehicle number %d  collisions occurred number %d collisions rate %s pT-m %0.4f s jerks %s lock_num %d" % (
        res["vehicles"], res["collisions"], res["collisions_rate"], res["pT_m"], res["jerk_mean"], res["lock_num"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mat", help="MATLAB v5 arrival stream (variable arvTimeNewVeh)")
    ap.add_argument("--synthetic", type=float, help="instead of --mat: synthetic Poisson arrivals at RATE veh/h/lane")
    ap.add_argument("--weights", required=True, help=".npz with the 12 actor tensors (tools/extract_actor.py)")
    ap.add_argument("--ticks", type=int, default=1000)
    ap.add_argument("--envs", type=int, default=1)
    ap.add_argument("--capacity", type=int, default=128, help="slots per intersection: 64, 128 or 256 (256: lane_num 12)")
    ap.add_argument("--vm", type=float, default=5.0)
    ap.add_argument("--lane-num", type=int, default=12, choices=(12, 8, 4), help="main.py --lane_num (:101)")
    ap.add_argument("--seed", type=int, default=20250213, help="synthetic streams / 8-lane intention draws")
    ap.add_argument("--rates", help="comma-separated veh/h/lane, e.g. 1200,1000,900,800,600,400,200: batch_test()'s densities in "
                                    "one batch of --envs environments each, streams generated on the device; one line per density")
    a = ap.parse_args()
    z = np.load(a.weights)
    weights = {k: z[k] for k in z.files}
    if a.rates:
        rates = [float(x) for x in a.rates.split(",") if x.strip()]
        results = evaluate_rates(rates, weights, ticks=a.ticks, envs_per_rate=a.envs, capacity=a.capacity, seed=a.seed, vm=a.vm,
                                 lane_num=a.lane_num)
        for res in results:
            print("rate %g veh/h/lane x %d envs" % (res["rate"], res["n_envs"]))
            print(rate_line(res))
        print(json.dumps(results))
        return
    if a.mat:
        arr = pad_stream(load_arrival_mat(a.mat))
    else:
        arr = synthetic_arrivals(a.envs, rate=a.synthetic or 1000.0, horizon_s=a.ticks * 0.1 + 30, seed=a.seed,
                                 lane_num=a.lane_num)
    if arr.shape[-1] != a.lane_num:
        ap.error("the arrival stream has %d columns, --lane-num is %d" % (arr.shape[-1], a.lane_num))
    draws = None
    if a.lane_num == 8:                        # the reference draws them with random.randint (ref :390)
        draws = synthetic_intentions(a.envs, arr.shape[-2], seed=a.seed)
        draws = draws if arr.ndim == 3 else draws[0]
    res = evaluate(arr, weights, ticks=a.ticks, n_envs=a.envs, capacity=a.capacity, vm=a.vm, lane_num=a.lane_num,
                   intentions=draws)
    print("vehicle number: %d; collisions occurred number: %d; collisions rate: %s" % (
        res["vehicles"], res["collisions"], res["collisions_rate"]))
    print("pT-m: %.3f s; mean jerk: %.3f; lock_num: %d; mean reward: %.4f" % (
        res["pT_m"], res["jerk_mean"], res["lock_num"], res["reward_mean"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
