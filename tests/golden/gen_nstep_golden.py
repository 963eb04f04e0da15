"""Generate tests/golden/nstep_ref.npz: the n-step transitions the UNMODIFIED reference environment produces under the
bookkeeping of its training loop (main.py:243-266), next to the same run's per-tick outputs in the layout of this project's
trajectory blocks.

Run in the build container only:   python tests/golden/gen_nstep_golden.py

The reference environment is driven through tests/golden/ref_harness.py.  Between scene_update() and delete_vehicle() every
vehicle of `ids` gets [state_now, actions, reward, state_next, Done] appended to ITS OWN veh["buffer"]; when it is Done or its
veh["count"] exceeds seq_max_step = 12 the rewards are folded backwards with gamma, gamma * Q' is added behind the last entry
unless Done, the oldest entry is emitted and popped and count is decremented -- exactly main.py:243-266, with two stated
differences: Q' is a RECORDED STAND-IN (a fixed float32 per tick and vehicle, stored in the fixture as q[tick][slot]) instead of
the target networks, and the fold is float64 explicitly (np.float64 operands; the type of the reference's own gamma * Q depends
on the NumPy version).  Two gammas are folded side by side: tanh(6 / 12) * 0.9 (main.py:227, epoch 0) and 0.8.

Stored (one intersection, K = 64 slots; slot = rank in (lane, j) order at tick start, as the C ABI defines it):
  reward, flags (ALIVE | CTL | DONE | DELETED bits), new_slot, ids (vehicle id per slot, -1 = empty)   [T][1][K]
  obs_first [1][K][28], row_t / row_slot / row_val: the non-empty rows of obs_post (veh["state"][0] after the tick)
  ctl_t / ctl_slot / ctl_col2: column 2 of the 7 state rows of every controlled vehicle (what state_pre holds there)
  q [T][1][K] float32, gammas [2], window = 13
  em_tick, em_id, em_row [M][28] (row 0 of s0), em_act [M][7], em_target [2][M]: the emitted transitions, in emission order
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle.record import get_policy  # noqa: E402
from tests.golden import ref_harness as rh  # noqa: E402

K, T, SEQ_MAX_STEP = 64, 300, 12
GAMMAS = np.array([np.tanh(6.0 / 12.0) * 0.9, 0.8], np.float64)
F_ALIVE, F_CTL, F_DONE, F_DELETED = 1, 2, 4, 8


class Runner(rh.RefRunner):
    """RefRunner with a hook between scene_update() and delete_vehicle() (where main.py:243-266 runs)."""

    def _snapshot(self, out):
        rec = rh.RefRunner._snapshot(self, out)
        self.hook(out)
        return rec


def slot_view(env):
    """(ids in slot order, lane starts) of the vehicles alive now"""
    ids, starts = [], []
    for lane in range(12):
        starts.append(len(ids))
        ids += [v["id_info"][0] for v in env.veh_info[lane]]
    return ids, starts


def main():
    arr = rh.load_stream("200")
    ref = Runner(arr, get_policy("sin1"), want_state=True, vm=6)
    env = ref.env
    rng = np.random.RandomState(20)
    q = rng.uniform(-30.0, 30.0, (T, 1, K)).astype(np.float32)
    reward = np.zeros((T, 1, K))
    flags = np.zeros((T, 1, K), np.int32)
    new_slot = np.full((T, 1, K), -1, np.int32)
    ids_at = np.full((T, 1, K), -1, np.int32)
    obs_post = np.zeros((T, 1, K, 28))
    ctl_t, ctl_slot, ctl_col2 = [], [], []
    em = dict(tick=[], id=[], row=[], act=[], target=[])
    cur = {}

    def hook(out):
        ids, state_next, rew, actions = out[0], out[1], out[2], out[3]
        t, state_now, pre_ids, starts = cur["t"], cur["state_now"], cur["ids"], cur["starts"]
        assert len(ids) == len(state_now)
        for seq, (lane, j) in enumerate(ids):
            veh = env.veh_info[lane][j]
            slot = starts[lane] + j
            assert pre_ids[slot] == veh["id_info"][0]
            # (what the device blocks hold for this slot)
            reward[t, 0, slot] = float(rew[seq])
            flags[t, 0, slot] |= F_CTL | (F_DONE if veh["Done"] else 0)
            st = np.array(state_next[seq], np.float64).reshape(7, 28)
            assert np.array_equal(st[:, 2], np.array(actions[seq], np.float64).reshape(7))       # ref :290
            ctl_t.append(t); ctl_slot.append(slot); ctl_col2.append(st[:, 2].copy())
            # main.py:243-266
            veh["buffer"].append([state_now[seq], actions[seq], rew[seq], state_next[seq], veh["Done"]])
            if veh["Done"] or veh["count"] > SEQ_MAX_STEP:
                seq_data = veh["buffer"]
                targets = []
                for gamma in GAMMAS:
                    if veh["Done"]:
                        r_target = np.float64(seq_data[-1][2])
                    else:
                        r_target = np.float64(seq_data[-1][2]) + gamma * np.float64(q[t, 0, slot])
                    for cur_data in reversed(seq_data[:-1]):
                        r_target = np.float64(cur_data[2]) + gamma * r_target
                    targets.append(r_target)
                em["tick"].append(t); em["id"].append(veh["id_info"][0])
                em["row"].append(np.array(seq_data[0][0], np.float64).reshape(7, 28)[0].copy())
                em["act"].append(np.array(seq_data[0][1], np.float64).reshape(7).copy())
                em["target"].append(targets)
                veh["buffer"].pop(0)
                veh["count"] -= 1
    ref.hook = hook
    obs_first = np.zeros((1, K, 28))
    pre_ids, _ = slot_view(env)
    for lane in range(12):
        for v in env.veh_info[lane]:
            assert not np.asarray(v["state"][0]).any()             # the constructor's vehicles have not been observed yet
    for t in range(T):
        pre_ids, starts = slot_view(env)
        assert len(pre_ids) <= K
        state_now = []
        for lane in range(12):
            for v in env.veh_info[lane]:
                if v["control"]:
                    state_now.append(np.array(v["state"], np.float64).copy())
        cur.update(t=t, state_now=state_now, ids=pre_ids, starts=starts)
        for s, vid in enumerate(pre_ids):
            ids_at[t, 0, s] = vid
            flags[t, 0, s] |= F_ALIVE
        ref.tick()
        post_ids, _ = slot_view(env)
        where = {vid: s for s, vid in enumerate(post_ids)}
        for s, vid in enumerate(pre_ids):
            new_slot[t, 0, s] = where.get(vid, -1)
            if vid not in where:
                flags[t, 0, s] |= F_DELETED
        s = 0
        for lane in range(12):
            for v in env.veh_info[lane]:
                obs_post[t, 0, s] = np.asarray(v["state"][0], np.float64)
                s += 1
    row_t, row_slot = np.nonzero(obs_post[:, 0].any(axis=-1))
    out = dict(T=T, K=K, window=SEQ_MAX_STEP + 1, gammas=GAMMAS, q=q, reward=reward, flags=flags, new_slot=new_slot, ids=ids_at,
               obs_first=obs_first, row_t=row_t.astype(np.int32), row_slot=row_slot.astype(np.int32), row_val=obs_post[row_t, 0, row_slot],
               ctl_t=np.array(ctl_t, np.int32), ctl_slot=np.array(ctl_slot, np.int32), ctl_col2=np.array(ctl_col2, np.float64),
               em_tick=np.array(em["tick"], np.int32), em_id=np.array(em["id"], np.int32), em_row=np.array(em["row"], np.float64),
               em_act=np.array(em["act"], np.float64), em_target=np.array(em["target"], np.float64).T.copy(),
               meta=np.array(json.dumps(dict(stream="200", policy="sin1", ctor=dict(vm=6), ticks=T, numpy=np.__version__,
                                             guard_hits=int(ref.guard_hits)))))
    path = os.path.join(HERE, "nstep_ref.npz")
    np.savez_compressed(path, **out)
    done = int(((flags & F_DONE) != 0).sum())
    print("nstep_ref.npz: %d ticks, %d controlled vehicle-ticks, %d Done, %d transitions -> %d KB"
          % (T, len(ctl_t), done, len(em["tick"]), os.path.getsize(path) // 1024))


if __name__ == "__main__":
    main()
