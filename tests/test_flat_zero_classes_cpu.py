"""Zero classes of the flat triangle list without a device: the lemma behind them (tests/cpp/flat_mt_fuzz.cpp on the kernels' own
header, csrc/ptk_flat_mt.h) and the classifier (ptk_flat_zero_class, the function classify_flat_kernel calls).

A class names edge words of a record that are stored as zeros; the exact PLAIN pass deletes the operations on them.  The fuzz
program holds every built mask to the full test: same accept decision, same bits of t for every accepted hit, u and v equal as
values, all-NaN directions rejected - on records whose masked words are +0 / -0 and whose other inputs mix ordinary values with
0, -0, +-1, denormals and 2^+-60.  It fails by itself when a mask sees fewer than 10 000 accepted hits."""
import os
import subprocess

import numpy as np
import pytest

import flat_zero_scenes as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbrpathtracer_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "flat_mt_fuzz.cpp")


def _build_and_run(tmp_path, name, flags, cases):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-I" + CSRC, SRC, "-o", exe] + flags)
    out = subprocess.run([exe, str(cases)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("ok") and out.stdout.count("mismatches accept 0 t 0 uv 0") == 32, out.stdout[-3000:]
    return out.stdout


def test_every_mask_accepts_the_same_hits_with_the_same_t(tmp_path):
    _build_and_run(tmp_path, "flat_mt_fuzz", ["-O2"], 200000)


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone host program: the sanitizers' runtime is linked into it, nothing is preloaded"""
    _build_and_run(tmp_path, "flat_mt_fuzz_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], 40000)


def _masks():
    from pbrpathtracer_amd import ptk
    return [ptk.flat_zero_mask(c) for c in range(16)]


def _classes(arrays):
    from pbrpathtracer_amd import ptk
    v = np.asarray(arrays["verts"], np.float32).reshape(-1, 3, 3)
    return [ptk.flat_zero_class(t[0], t[1], t[2]) for t in v]


def test_the_built_masks():
    from pbrpathtracer_amd import ptk
    m = _masks()
    assert m[0] == 0 and m[1:4] == [9, 18, 36] and len(set(m)) == 16
    for c in range(4, 16):
        assert bin(m[c]).count("1") == 3 and any(m[c] & p == p for p in (9, 18, 36)), (c, m[c])
        assert m[c] & 7 != 7 and m[c] & 56 != 56
    assert ptk.flat_zero_mask(-1) == -1 and ptk.flat_zero_mask(16) == -1


def test_class_is_the_largest_built_subset_of_the_zero_set():
    from pbrpathtracer_amd import ptk
    L = ptk.load()
    import ctypes as C
    m = _masks()
    rng = np.random.default_rng(11)
    seen = set()
    for _ in range(8000):
        e = rng.normal(0, 1, 6).astype(np.float32)
        z = rng.random(6) < rng.choice([0.2, 0.5, 0.8])
        e[z] = np.where(rng.random(int(z.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))      # -0 counts as zero
        zset = sum(1 << k for k in range(6) if e[k] == 0)
        c = int(L.ptk_flat_zero_class((C.c_float * 6)(*e.tolist())))
        seen.add(c)
        assert m[c] & ~zset == 0, (e, c)
        if zset & 7 == 7 or zset & 56 == 56:
            assert c == 0, (e, c)                       # an edge that is all zero: degenerate, general
            continue
        fits = [k for k in range(16) if m[k] & ~zset == 0]
        most = max(bin(m[k]).count("1") for k in fits)
        assert c == min(k for k in fits if bin(m[k]).count("1") == most), (e, c, fits)
    assert seen == set(range(16))
    assert L.ptk_flat_zero_class(None) == 0


def test_denormal_words_are_not_zero():
    from pbrpathtracer_amd import ptk
    tiny = np.float32(1e-42)
    assert ptk.flat_zero_class((0, 0, 0), (1, tiny, 0), (1, tiny, 1)) == 0
    assert ptk.flat_zero_class((0, 0, 0), (1, -0.0, 0), (1, 0.0, 1)) != 0


def test_scenes_reach_every_class():
    """the Cornell box of C2: twelve three-zero records; turned 30 degrees about a skew axis: twelve general ones; across the test
    scenes every built class is selected (the GPU test asserts the same of the device's table)"""
    m = _masks()
    s = Z.all_scenes()
    box = _classes(s["cornell"])
    assert len(box) == 12 and all(c >= 4 for c in box), box
    assert _classes(s["skewed"]) == [0] * 12
    assert all(1 <= c <= 3 for c in _classes(s["in-plane"])) and set(_classes(s["in-plane"])) == {1, 2, 3}
    mix = _classes(s["mixed"])
    assert 0 in mix and any(1 <= c <= 3 for c in mix) and any(c >= 4 for c in mix)
    assert len(_classes(s["one"])) == 1 and len(_classes(s["sixteen"])) == 16 and all(c >= 4 for c in _classes(s["sixteen"]))
    reached = set()
    for name, a in s.items():
        e = Z.edges(a)
        for k, c in enumerate(_classes(a)):
            zset = sum(1 << b for b in range(6) if e[k, b] == 0)
            assert m[c] & ~zset == 0, (name, k)
            reached.add(c)
    assert reached == set(range(16)), sorted(set(range(16)) - reached)
