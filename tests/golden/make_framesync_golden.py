"""Writes tests/golden/framesync_ref_vectors.npz: the unmodified reference's `csdr pattern_search_u8_u8` on a dozen small cases (pattern, values_after, input
bytes, its stdout).  Data only.  Run from the repository root where oracle/_ref/csdr exists:
    python tests/golden/make_framesync_golden.py"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import framesync_model as fm  # noqa: E402


def planted(seed, pat, V, n, alphabet):
    """n random bytes with the pattern planted at random gaps"""
    rng = np.random.default_rng(seed)
    pat = np.asarray(pat, np.uint8)
    x = rng.integers(0, alphabet, n).astype(np.uint8)
    at = int(rng.integers(0, 2 * pat.size + 3))
    while at + pat.size <= n:
        x[at:at + pat.size] = pat
        at += pat.size + int(rng.integers(0, 3 * (pat.size + V) + 2))
    return x


def framed(seed, pat, alphabet, layout):
    """the stream that `layout` spells: an int g is g bytes of filler that cannot hold the pattern's first value, "p" the pattern, ("d", k) k random bytes"""
    rng = np.random.default_rng(seed)
    pat = np.asarray(pat, np.uint8)
    other = [v for v in range(alphabet) if v != int(pat[0])]
    parts = []
    for it in layout:
        parts.append(pat if it == "p" else rng.integers(0, alphabet, it[1]).astype(np.uint8) if isinstance(it, tuple) else rng.choice(other, it).astype(np.uint8))
    return np.concatenate(parts)


def cases():
    rng = np.random.default_rng(77)
    bits16 = rng.integers(0, 2, 16)
    bytes33 = rng.integers(0, 255, 33)
    P5, B16 = [2, 0, 1, 1, 0], np.r_[1, bits16[1:]]         # (first values that the filler can avoid)
    c = [
        ("one_value", [1], 0, planted(1, [1], 0, 300, 3)),
        ("one_value_payload", [7], 7, planted(2, [7], 7, 600, 256)),
        ("two_bits", [1, 0], 1, planted(3, [1, 0], 1, 500, 2)),
        ("five_bytes", [3, 1, 4, 1, 5], 7, planted(4, [3, 1, 4, 1, 5], 7, 1200, 256)),
        ("sixteen_bits", bits16, 64, planted(5, bits16, 64, 3000, 2)),
        ("thirtythree_bytes", bytes33, 300, planted(6, bytes33, 300, 4000, 256)),
        ("ones_overlap", [1, 1, 1], 1, planted(7, [1, 1, 1], 1, 600, 2)),
        ("alternating_overlap", [0, 1, 0, 1], 7, planted(8, [0, 1, 0, 1], 7, 900, 2)),
        # A searcher (re)started at s with ring index 0 compares x[s .. s+L-1] when x[s+L] arrives and drops x[s+L].  The first pattern lies at the stream's
        # start, one byte behind it the payload; the next pattern begins right behind that payload and is found the same way, and so on.
        ("frame_behind_payload", P5, 7, framed(9, P5, 3, ["p", 1, ("d", 7)] * 4 + [30])),
        # the same with one byte between a payload and the next pattern: the pattern then holds the byte that the restarted searcher drops and is lost
        ("pattern_one_late", P5, 7, framed(10, P5, 3, ["p", 1, ("d", 7)] + [1, "p", 1, ("d", 7)] * 3 + [30])),
        # matches at arbitrary distances, so that restarts carry a ring index other than 0, with patterns right behind the payloads and later
        ("carried_index", P5, 7, framed(11, P5, 3, [8, "p", ("d", 7), "p", ("d", 7), 4, "p", ("d", 7), 1, "p", ("d", 7), 13, "p", ("d", 7), "p", ("d", 7), 6,
                                                    "p", ("d", 7), 2, "p", ("d", 7), 30])),
        ("carried_index_long", B16, 64, framed(12, B16, 2, [21, "p", ("d", 64), "p", ("d", 64), 40, "p", ("d", 64), 3, "p", ("d", 64), 23, "p", ("d", 64), 17,
                                                            "p", ("d", 64), 70])),
    ]
    return c


def main():
    if fm.ref_cli() is None:
        raise SystemExit("oracle/_ref/csdr is not built")
    out, names = {}, []
    for k, (name, pat, V, x) in enumerate(cases()):
        pat = np.asarray(pat, np.uint32)
        assert pat[-1] != 255                                # the reference takes the end of file for a byte 0xFF, which could complete a match there
        names.append(name)
        out["pat%d" % k], out["V%d" % k], out["x%d" % k] = pat, np.int32(V), x
        out["y%d" % k] = fm.ref_search(pat, V, x)
        print("%-22s L %2d V %3d n %4d -> %4d bytes" % (name, pat.size, V, x.size, out["y%d" % k].size))
    out["names"] = np.array(names)
    np.savez_compressed(fm.GOLDEN, **out)
    print(fm.GOLDEN, os.path.getsize(fm.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
