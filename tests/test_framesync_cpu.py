"""The frame synchroniser without a GPU: the Python definition (tests/framesync_model.py) against the unmodified reference's recorded output and, where it is
built, its binary; the library's CPU walk (the kernels' step function) against the definition bit for bit, with positions and final state, over call cuts and
mismatch allowances; the record's round trip; create errors; the ABI."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest

import csdr_amd
import framesync_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["csdr_amd_framesync_create", "csdr_amd_framesync_process", "csdr_amd_framesync_max_out", "csdr_amd_framesync_max_frames", "csdr_amd_framesync_tile",
           "csdr_amd_framesync_reset", "csdr_amd_framesync_reset_channel", "csdr_amd_framesync_get_channel", "csdr_amd_framesync_set_channel",
           "csdr_amd_framesync_set_lanes", "csdr_amd_framesync_lanes", "csdr_amd_framesync_force_generic", "csdr_amd_framesync_kernel_name",
           "csdr_amd_framesync_destroy", "csdr_amd_pattern_search_u8_u8", "csdr_amd_debug_framesync_walk"]


@pytest.fixture(scope="module")
def golden():
    g = np.load(fm.GOLDEN)
    return [(str(nm), g["pat%d" % k], int(g["V%d" % k]), g["x%d" % k], g["y%d" % k]) for k, nm in enumerate(g["names"])]


def cut_sets(L, V, x, pos):
    """call cuts of 0, 1, L-1, L, L+1 bytes (the byte behind the first L alone in a call), 2L, 2L+1, inside a payload and at its last byte"""
    sets = [[], [0, 1, 0, 1], [L - 1, 1, 1], [L, 1, L, 1], [L + 1], [2 * L, 1], [2 * L + 1, 0, 1], [1] * min(x.size, 3 * L + 4)]
    if len(pos) and V > 0:
        p = int(pos[0])
        sets += [[p + V // 2, 1], [p + V - 1, 1], [p + V]]
    elif len(pos):
        sets += [[int(pos[0]) - 1, 1], [int(pos[0])]]
    return sets


def walk(pat, V, x, m=0, cuts=()):
    st, w = csdr_amd.FrameSyncChan(), np.zeros(len(pat), np.uint8)
    out, pos = csdr_amd.framesync_debug_walk(pat, V, x, m, cuts, st, w)
    return out, pos, st.astuple()


def test_the_golden_file_holds_the_cases(golden):
    names = [g[0] for g in golden]
    assert len(names) >= 12 and {"frame_behind_payload", "pattern_one_late", "carried_index", "ones_overlap", "alternating_overlap"} <= set(names)
    assert {g[1].size for g in golden} >= {1, 2, 5, 16, 33} and {g[2] for g in golden} >= {0, 1, 7, 64, 300}
    assert os.path.getsize(fm.GOLDEN) < 100 * 1024


def test_model_against_the_recorded_reference(golden):
    """on whole frames: the model's complete frames lead the reference's stdout, which may add one block of V bytes (its write after a short fread)"""
    for name, pat, V, x, y in golden:
        frames = fm.whole_frames(pat, V, x)
        assert fm.leads(frames, y, V), name
        assert frames.size > 0 or V == 0, name


def test_what_the_special_cases_show(golden):
    """a pattern right behind a payload is found by a searcher restarted with index 0; one byte later it holds the dropped byte and is lost"""
    by = {g[0]: g for g in golden}
    _, pat, V, x, _ = by["frame_behind_payload"]
    assert len(fm.search(pat, V, x)[1]) == 4
    _, pat, V, x, _ = by["pattern_one_late"]
    planted = sum(1 for i in range(x.size - pat.size + 1) if np.array_equal(x[i:i + pat.size], pat.astype(np.uint8)))
    assert planted == 4 and len(fm.search(pat, V, x)[1]) < planted


def test_model_against_the_reference_binary():
    if fm.ref_cli() is None:
        pytest.skip("the reference binary is not built on this host")
    rng = np.random.default_rng(2024)
    for it in range(60):
        L, V = int(rng.integers(1, 12)), int(rng.integers(0, 20))
        pat, x = fm.random_case(rng, L, V, [2, 3, 256][it % 3], int(rng.integers(20, 1200)), plant=it % 4 != 0)
        assert fm.leads(fm.whole_frames(pat, V, x), fm.ref_search(pat, V, x), V), (it, L, V)


@pytest.mark.parametrize("m", [0, 1, 3])
def test_walk_equals_the_model(golden, m):
    for name, pat, V, x, _ in golden:
        if m >= pat.size:
            continue
        want = fm.search(pat, V, x, m)
        for cuts in cut_sets(pat.size, V, x, want[1]):
            o, p, st = walk(pat, V, x, m, cuts)
            assert np.array_equal(o, want[0]) and np.array_equal(p, want[1]) and st == want[2], (name, m, cuts)
            mo, mp, mst = fm.search(pat, V, x, m, cuts)
            assert np.array_equal(mo, want[0]) and np.array_equal(mp, want[1]) and mst == want[2], (name, m, cuts)


def test_walk_equals_the_model_on_random_streams():
    rng = np.random.default_rng(7)
    for it in range(120):
        L, V = int(rng.integers(1, 40)), int(rng.integers(0, 50))
        m = int(rng.integers(0, min(L, 4)))
        pat, x = fm.random_case(rng, L, V, [2, 3, 256][it % 3], int(rng.integers(0, 1500)))
        cuts = rng.integers(0, 2 * L + 3, int(rng.integers(0, 9))).tolist()
        want = fm.search(pat, V, x, m)
        o, p, st = walk(pat, V, x, m, cuts)
        assert np.array_equal(o, want[0]) and np.array_equal(p, want[1]) and st == want[2], (it, L, V, m)


def test_a_mismatch_allowance_finds_damaged_patterns():
    rng = np.random.default_rng(5)
    pat = rng.integers(0, 2, 24)
    x = np.zeros(400, np.uint8)
    x[100:124] = pat; x[103] ^= 1; x[117] ^= 1
    x[124:140] = 1
    assert len(walk(pat, 16, x, 0)[1]) == 0 and len(walk(pat, 16, x, 1)[1]) == 0
    o, p, _ = walk(pat, 16, x, 2)
    assert p.tolist() == [124] and np.array_equal(o, x[124:140])


def test_state_round_trip(golden):
    """a stream processed half with one record and half with a copy of it (and of its ring) equals the uncut stream"""
    for name, pat, V, x, _ in golden:
        want = fm.search(pat, V, x)
        for half in (x.size // 2, x.size // 3, pat.size, pat.size + 1):
            st, w = csdr_amd.FrameSyncChan(), np.zeros(pat.size, np.uint8)
            o1, p1 = csdr_amd.framesync_debug_walk(pat, V, x[:half], 0, (), st, w)
            st2, w2 = csdr_amd.FrameSyncChan.from_buffer_copy(bytes(st)), w.copy()
            o2, p2 = csdr_amd.framesync_debug_walk(pat, V, x[half:], 0, (), st2, w2)
            assert np.array_equal(np.concatenate([o1, o2]), want[0]) and np.array_equal(np.concatenate([p1, p2]), want[1]), (name, half)
            assert st2.astuple() == want[2]


def test_walk_rejects_what_create_rejects():
    x = np.zeros(8, np.uint8)
    for pat, V, m in (([], 1, 0), ([0] * 1025, 1, 0), ([1, 2], -1, 0), ([1, 2], (1 << 30) + 1, 0), ([1, 2], 1, 2), ([1, 2], 1, -1), ([1, 256], 1, 0)):
        with pytest.raises(csdr_amd.CsdrAmdError):
            csdr_amd.framesync_debug_walk(pat, V, x, m)
    st = csdr_amd.FrameSyncChan(fill=3, index=1)                 # an index behind the fill count: no stream leads there
    with pytest.raises(csdr_amd.CsdrAmdError):
        csdr_amd.framesync_debug_walk([1, 2, 3, 4], 1, x, 0, (), st, np.zeros(4, np.uint8))
    assert csdr_amd.framesync_debug_walk([1] * 1024, 1 << 30, x)[0].size == 0
    with pytest.raises(csdr_amd.CsdrAmdError, match="above 255"):
        csdr_amd.framesync_debug_walk([300], 1, x)


def test_symbols_are_exported_and_declared():
    out = subprocess.run(["nm", "-D", "--defined-only", csdr_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not sorted(set(SYMBOLS) - exported)
    txt = open(os.path.join(ROOT, "include", "csdr_amd.h")).read()
    for n in SYMBOLS:
        assert n + "(" in txt, n


def test_record_sizes_agree(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "csdr_amd.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(csdr_amd_framesync_chan), '
                   'offsetof(csdr_amd_framesync_chan, remain), offsetof(csdr_amd_framesync_chan, base), offsetof(csdr_amd_framesync_chan, frames)); return 0; }\n')
    exe = str(tmp_path / "s")
    r = subprocess.run(["gcc", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    T = csdr_amd.FrameSyncChan
    assert got == [C.sizeof(T), T.remain.offset, T.base.offset, T.frames.offset] == [32, 8, 16, 24]
