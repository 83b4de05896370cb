"""The definition of the frame synchroniser (csdr_amd_framesync, `csdr pattern_search_u8_u8`, csdr.c:3532-3597) as plain integer Python: one stream, the
state carried across calls, so that the result does not depend on how calls cut the stream.

It is the reference's loop, byte by byte.  A ring of L bytes, a write index and a fill count.  Every byte is stored at the index, which then moves on
(csdr.c:3555); while fewer than L bytes have come since the (re)start nothing else happens (csdr.c:3556).  Otherwise the index wraps to 0 at L and the ring,
read from the index on, is compared with the pattern (csdr.c:3557-3585).  A match (at most max_mismatch positions differ) at byte p emits x[p+1 .. p+V] and
restarts the FILL COUNT ONLY at p+V+1 (csdr.c:3590): the index stays where the match left it, k = (p - s - L) mod L for a searcher started at s.  What
follows from that, for a restart at s with index k:
  - x[s .. s+L-k-1] go to ring[k .. L-1]; the k + 1 bytes x[s+L-k .. s+L] land at and past the ring's end, where the reference writes beyond its buffer and
    nothing reads them: they are dropped.  x[s+L] triggers the first check.
  - ring[0 .. k-1] still hold the last k bytes of the window that matched, so the first k checks see them in front of the new bytes.
  - With k = 0 (always so after a reset, and whenever a match comes L bytes after the first check or a multiple of L later) the pattern at s is found and
    only x[s+L] is dropped.
Here a store past the ring is left out; everything else is the reference's.

Also here: the helpers that run the unmodified reference binary where oracle/_ref/csdr exists, and the path of the golden file recorded from it."""
import os
import subprocess
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "framesync_ref_vectors.npz")


class FrameSyncModel:
    def __init__(self, pattern, values_after, max_mismatch=0):
        self.pat = [int(v) for v in pattern]
        self.L, self.V, self.m = len(self.pat), int(values_after), int(max_mismatch)
        assert self.L >= 1 and self.V >= 0 and 0 <= self.m < self.L
        self.ring = [0] * self.L
        self.reset()

    def reset(self):
        self.fill = 0          # bytes since the (re)start, L at most
        self.index = 0         # where the next byte is stored: 0 .. L-1 while checking, k .. k+L while the ring fills
        self.remain = 0        # payload bytes left to copy
        self.base = 0          # absolute index of the next byte
        self.frames = 0

    def state(self):
        return (self.fill, self.index, self.remain, self.base, self.frames)

    def process(self, x):
        """-> (payload bytes of this call, absolute index of each match's first payload byte)"""
        out, pos = [], []
        L = self.L
        for b in np.asarray(x, np.uint8).tolist():
            p = self.base
            self.base += 1
            if self.remain > 0:
                out.append(b)
                self.remain -= 1
                continue
            if self.index < L:
                self.ring[self.index] = b
            self.index += 1
            if self.fill < L:
                self.fill += 1
                continue
            if self.index >= L:
                self.index = 0
            w = self.ring[self.index:] + self.ring[:self.index]
            if sum(1 for a, c in zip(w, self.pat) if a != c) <= self.m:
                self.frames += 1
                pos.append(p + 1)
                self.remain, self.fill = self.V, 0
        return np.array(out, np.uint8), np.array(pos, np.int64)


def search(pattern, values_after, x, max_mismatch=0, cuts=()):
    """the whole stream x cut into calls of cuts[0], cuts[1], ... bytes and the rest -> (payload, positions, final state)"""
    mdl = FrameSyncModel(pattern, values_after, max_mismatch)
    x = np.asarray(x, np.uint8)
    outs, poss, done = [], [], 0
    for c in list(cuts) + [x.size]:
        c = min(max(int(c), 0), x.size - done)
        o, p = mdl.process(x[done:done + c])
        outs.append(o); poss.append(p); done += c
    return np.concatenate(outs), np.concatenate(poss), mdl.state()


def whole_frames(pattern, values_after, x, max_mismatch=0):
    """the payloads that arrived completely, concatenated"""
    out, pos, _ = search(pattern, values_after, x, max_mismatch)
    n = sum(1 for p in pos.tolist() if p + values_after <= len(x))
    return out[:n * values_after]


def ref_cli():
    import oracle
    return oracle.REF_CLI if os.path.exists(oracle.REF_CLI) else None


def ref_search(pattern, values_after, x):
    """stdout of the unmodified reference's `csdr pattern_search_u8_u8` fed x through a pipe"""
    argv = [ref_cli(), "pattern_search_u8_u8", str(int(values_after))] + [str(int(v)) for v in pattern]
    r = subprocess.run(argv, input=np.asarray(x, np.uint8).tobytes(), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=60)
    return np.frombuffer(r.stdout, np.uint8)


def leads(model_frames, ref_out, values_after):
    """The comparison on whole frames: the model's complete frames lead the reference's output, which may add at most one block of values_after bytes behind
    them (its write after a short fread at end of file)."""
    n = model_frames.size
    return ref_out.size in (n, n + values_after) and np.array_equal(ref_out[:n], model_frames)


def random_case(rng, L, V, alphabet, n, plant=True):
    """(pattern, x): n bytes from range(alphabet) with the pattern planted at random gaps; the pattern's last value is kept below 255"""
    pat = rng.integers(0, alphabet, L).astype(np.uint8)
    pat[-1] = min(int(pat[-1]), 254)
    x = rng.integers(0, alphabet, n).astype(np.uint8)
    at = int(rng.integers(0, 2 * L + 3))
    while plant and at + L <= n:
        x[at:at + L] = pat
        at += L + int(rng.integers(0, 3 * (L + V) + 2))
    return pat, x
