"""The reference's n-step bookkeeping (main.py:243-266), keyed by VEHICLE ID: the arbiter of the slot-indexed device pass.

Plain Python / NumPy that knows nothing about slots, links or blocks.  Every vehicle id owns a buffer of at most `window` =
seq_max_step + 1 entries (s0 row [28], act7 [7], reward, q, done).  feed() is called tick by tick with the controlled vehicles
of that tick; when a vehicle's buffer is full or its newest entry is Done the rewards are folded in float64, every operation
rounded on its own, in the reference's backward order

    r = r_last (+ gamma * float64(q_last) unless Done);    r = r_k + gamma * r    for the older entries, newest first

and the OLDEST entry is emitted with that target.  On Done the younger entries are dropped with the vehicle (tail=True emits
them too, each folded over the entries behind it, as the device pass's NSTEP_TAIL does); after a full window the oldest entry
slides out.  tests/test_nstep_identity.py pins this to tests/golden/nstep_ref.npz (the unmodified reference under its own
buffers, tests/golden/gen_nstep_golden.py), bit for bit."""
import collections

import numpy as np

Emission = collections.namedtuple("Emission", "tick vid row act7 target entries boot done")


def fold(entries, gamma, done):
    """entries: (reward, q) oldest first -> the float64 target of the oldest"""
    gamma = np.float64(gamma)
    r = np.float64(entries[-1][0])
    if not done:
        gq = gamma * np.float64(np.float32(entries[-1][1]))
        r = r + gq
    for rew, _ in reversed(entries[:-1]):
        gr = gamma * r
        r = np.float64(rew) + gr
    return r


class VehicleBuffers:
    def __init__(self, gamma, window=13, tail=False):
        self.gamma, self.window, self.tail = np.float64(gamma), int(window), bool(tail)
        self.buf = {}                                  # vehicle id -> list of (row, act7, reward, q)
        self.out = []                                  # Emission, in emission order

    def feed(self, tick, vid, row, act7, reward, q, done):
        """One controlled vehicle at one tick: the row the actor consumed (s0), its 7 actions, its reward, the bootstrap Q' of
        this tick (float32; read only if a window closes here without Done) and whether the tick ended it (Done)."""
        vid, done = int(vid), bool(done)
        b = self.buf.setdefault(vid, [])
        b.append((np.array(row, np.float64), np.array(act7, np.float64), np.float64(reward), np.float32(q)))
        assert len(b) <= self.window
        if done or len(b) == self.window:
            starts = range(len(b)) if (done and self.tail) else (0,)
            for k in starts:
                part = b[k:]
                target = fold([(e[2], e[3]) for e in part], self.gamma, done)
                self.out.append(Emission(int(tick), vid, part[0][0], part[0][1], target, len(part), not done, done))
            b.pop(0)
        if done:
            del self.buf[vid]

    def emitted(self):
        """{(closing tick, vehicle id, entries used): Emission}; without tail, one emission per (closing tick, vehicle id)"""
        out = {}
        for em in self.out:
            key = (em.tick, em.vid, em.entries)
            assert key not in out, "emitted twice: %r" % (key,)
            out[key] = em
        if not self.tail:
            assert len({k[:2] for k in out}) == len(out)
        return out
