"""Window excursions on the CPU: the numpy reference against a plain loop, the monoid's
combine over every cut, the invariants that tie the record to the le-buckets, the argument
checks, the exposition, the compile-time resources of csrc/window_excursions.hip and the
host-only sanitizer program over the device's own combine header. No GPU."""

import os
import shutil
import subprocess

import numpy as np
import pytest

from rocmdash.ops.window_excursions import (
    E_ABOVE,
    E_CURRENT,
    E_EPISODES,
    E_LEADING,
    E_LONGEST,
    E_ROWS,
    E_SINCE,
    E_VALID,
    IDENTITY,
    MAX_THRESHOLDS,
    check_thresholds,
    default_thresholds,
    excursion_combine,
    parse_fractions,
    partial_of_record,
    record_of_partial,
    window_excursions_reference,
)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LDS_BYTES_PER_CU = 160 * 1024
VGPRS_FOR_4_WAVES = 128  # 512 per SIMD lane / 4 waves


def _loop(rows, t):
    """The semantics as a loop over the samples, one at a time."""
    n, S = rows.shape
    out = np.zeros((S, t.shape[1], 8), np.int32)
    for s in range(S):
        for k in range(t.shape[1]):
            above = valid = episodes = longest = run = since = 0
            leading = None
            for x in rows[:, s]:
                if x != x:
                    continue
                valid += 1
                if x > t[s, k]:
                    above += 1
                    run += 1
                    episodes += run == 1
                    longest = max(longest, run)
                    since = 0
                else:
                    if leading is None:
                        leading = run
                    run = 0
                    since += 1
            out[s, k] = [above, valid, episodes, longest, run, since, run if leading is None else leading, n]
    return out


def _random_rows(rng, n, S, t):
    """Random rows with NaN, +-inf and samples exactly on a threshold, in runs."""
    pool = np.concatenate([t.reshape(-1), [np.nan, np.nan, np.inf, -np.inf, -1e30, 1e30], rng.normal(1.0, 1.5, 12)])
    x = rng.choice(pool.astype(np.float32), size=(n, S))
    hold = rng.random((n, S)) < 0.6  # repeat the sample above: runs longer than one
    for i in range(1, n):
        x[i] = np.where(hold[i], x[i - 1], x[i])
    return x


T3 = np.array([[0.0, 1.0, 2.5], [-1.0, 0.5, 1.0], [1.0, 2.0, 3.0]], np.float32)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 17, 64, 400])
def test_reference_equals_the_loop(n):
    rng = np.random.default_rng(n)
    for _ in range(5):
        rows = _random_rows(rng, n, 3, T3)
        np.testing.assert_array_equal(window_excursions_reference(rows, T3), _loop(rows, T3))


def test_reference_edge_cases():
    t = np.array([[1.0, 2.0]], np.float32)
    ref = lambda v: window_excursions_reference(np.asarray(v, np.float32).reshape(-1, 1), t)[0]
    assert (ref([]) == 0).all()
    np.testing.assert_array_equal(ref([1.5]), [[1, 1, 1, 1, 1, 0, 1, 1], [0, 1, 0, 0, 0, 1, 0, 1]])
    np.testing.assert_array_equal(ref([1.0]), [[0, 1, 0, 0, 0, 1, 0, 1]] * 2)  # equal is not above
    np.testing.assert_array_equal(ref([np.nan] * 7), [[0, 0, 0, 0, 0, 0, 0, 7]] * 2)
    np.testing.assert_array_equal(ref([3.0] * 9), [[9, 9, 1, 9, 9, 0, 9, 9]] * 2)
    np.testing.assert_array_equal(ref([0.0] * 9), [[0, 9, 0, 0, 0, 9, 0, 9]] * 2)
    np.testing.assert_array_equal(ref([3.0, 0.0] * 4), [[4, 8, 4, 1, 0, 1, 1, 8]] * 2)
    np.testing.assert_array_equal(ref([0.0, 3.0] * 4), [[4, 8, 4, 1, 1, 0, 0, 8]] * 2)
    # NaN neither ends nor extends an episode; +inf is above, -inf is not
    np.testing.assert_array_equal(ref([np.inf, np.nan, 1.5, np.nan, -np.inf, 5.0, np.nan]),
                                  [[3, 4, 2, 2, 1, 0, 2, 7], [2, 4, 2, 1, 1, 0, 1, 7]])


@pytest.mark.parametrize("n", [0, 1, 5, 90])
def test_combine_over_every_cut_and_three_parts(n):
    """Folding the references of the parts with the combine is the reference of the whole:
    every cut position (empty sides included: the identity), and three parts at random
    positions under both bracketings (associativity)."""
    rng = np.random.default_rng(100 + n)
    rows = _random_rows(rng, n, 3, T3)
    whole = window_excursions_reference(rows, T3)

    def parts(*cuts):
        edges = (0,) + cuts + (n,)
        return [window_excursions_reference(rows[a:b], T3) for a, b in zip(edges, edges[1:])]

    cuts3 = [tuple(sorted(rng.integers(0, n + 1, 2))) for _ in range(30)]
    for cuts in [(c,) for c in range(n + 1)] + cuts3:
        ps = parts(*cuts)
        for s in range(3):
            for k in range(3):
                p = [partial_of_record(q[s, k]) for q in ps]
                left = p[0]
                for q in p[1:]:
                    left = excursion_combine(left, q)
                np.testing.assert_array_equal(record_of_partial(left, n), whole[s, k], err_msg=f"cuts {cuts}")
                if len(p) == 3:
                    right = excursion_combine(p[0], excursion_combine(p[1], p[2]))
                    assert right == left
                assert excursion_combine(IDENTITY, left) == left == excursion_combine(left, IDENTITY)


def test_combine_is_not_commutative():
    up, down = (1, 1, 1, 1, 1, 1, 0), (1, 0, 0, 0, 0, 0, 1)
    assert excursion_combine(up, down) != excursion_combine(down, up)


def test_invariants():
    from rocmdash.ops.window_buckets import window_buckets_reference

    rng = np.random.default_rng(9)
    for n in (1, 33, 500):
        rows = _random_rows(rng, n, 3, T3)
        r = window_excursions_reference(rows, T3).astype(np.int64)
        le = window_buckets_reference(rows.T, T3)  # [S, K + 1]: <= each bound, then the valid count
        np.testing.assert_array_equal(r[:, :, E_ABOVE], le[:, -1:] - le[:, :-1])
        np.testing.assert_array_equal(r[:, :, E_VALID], np.broadcast_to(le[:, -1:], (3, 3)))
        assert (np.diff(r[:, :, E_ABOVE], axis=1) <= 0).all()
        assert (np.diff((r[:, :, E_EPISODES] > 0).astype(int), axis=1) <= 0).all()
        assert (r[:, :, E_SINCE][r[:, :, E_CURRENT] > 0] == 0).all()
        none = r[:, :, E_EPISODES] == 0
        np.testing.assert_array_equal(r[:, :, E_SINCE][none], r[:, :, E_VALID][none])
        assert (r[:, :, E_LONGEST] >= np.maximum(r[:, :, E_CURRENT], r[:, :, E_LEADING])).all()
        assert (r[:, :, E_ROWS] == n).all()


@pytest.mark.parametrize("bad", [
    [], [[1.0, 2.0, 3.0, 4.0, 5.0]], [[1.0, 1.0]], [[2.0, 1.0]], [[np.nan]], [[1.0, np.inf]], [[-np.inf, 0.0]],
    [[[1.0]]], [[1.0], [2.0], [3.0]],  # 3 rows for 2 series
    [[1.0, np.float32(1.0) + 1e-9]],  # equal in fp32
])
def test_check_thresholds_rejects(bad):
    with pytest.raises(ValueError):
        check_thresholds(np.asarray(bad, dtype=np.float64), 2 if np.ndim(bad) == 2 and len(bad) == 3 else None)


def test_check_thresholds_accepts_and_broadcasts():
    t = check_thresholds([1.0, 2.0], 3)
    assert t.shape == (3, 2) and t.dtype == np.float32 and t.flags.c_contiguous
    assert check_thresholds(np.arange(MAX_THRESHOLDS)[None] + 0.5).shape == (1, MAX_THRESHOLDS)


@pytest.mark.parametrize("bad", ["", "0", "0.5,0.5", "0.9,0.5", "1.1", "-0.1", "a", "0.1,0.2,0.3,0.4,0.5", "nan", "0.5,,0.9",
                                 (), (0.5, 0.2)])
def test_fraction_parsing_rejects(bad):
    with pytest.raises(ValueError):
        parse_fractions(bad)


def test_fraction_parsing_and_default_thresholds():
    from rocmdash.ops.window_buckets import default_bounds

    assert parse_fractions("0.5, 0.9") == (0.5, 0.9) and parse_fractions("1") == (1.0,)
    assert parse_fractions((0.25, 0.5, 0.75, 1.0)) == (0.25, 0.5, 0.75, 1.0)
    series = ("amd_gpu_average_package_power", "amd_gpu_junction_temperature", "amd_gpu_used_vram")
    t = default_thresholds(series, 1400.0, 1000.0)
    axis = default_bounds(series, 1400.0, 1000.0, buckets=1)[:, 0]
    np.testing.assert_allclose(t, axis[:, None] * np.array([0.5, 0.75, 0.9]), rtol=1e-6)
    assert t.shape == (3, 3) and t[0, 0] == 700.0 and t[2, 2] == 900.0
    with pytest.raises(ValueError):
        default_thresholds(series, 1400.0, 1000.0, fractions=(0.9, 0.5))


SERIES = ("amd_gpu_average_package_power", "amd_gpu_junction_temperature")


def _snap(excursions=False):
    from rocmdash.models.schema import NUM_STATS
    from rocmdash.viz.panels import NodeSnapshot

    snap = NodeSnapshot(gpu_ids=["0", "1"], card_models=["102-G36236-0C"] * 2, columns=SERIES,
                        values=[[500.0, 70.0], [900.0, 80.0]], window=np.ones((2, 2, NUM_STATS)), window_series=SERIES)
    if excursions:
        rng = np.random.default_rng(4)
        thr = np.array([[700.0, 1260.0], [55.0, 99.0]], np.float32)
        x = rng.normal([[[800.0], [75.0]]], [[[300.0], [15.0]]], (2, 2, 256)).astype(np.float32)
        snap.window_excursions = np.stack([window_excursions_reference(x[g].T, thr) for g in range(2)])
        snap.window_excursion_thresholds = thr
    return snap


FAMILIES = {"rocmdash_window_excursions": E_EPISODES, "rocmdash_window_excursion_longest_samples": E_LONGEST,
            "rocmdash_window_excursion_current_samples": E_CURRENT, "rocmdash_window_excursion_since_samples": E_SINCE,
            "rocmdash_window_above_samples": E_ABOVE}


def test_render_snapshot_unchanged_without_excursions():
    from rocmdash.prom.exposition import render_snapshot

    never = _snap()
    text = render_snapshot(never, hostname="n1")
    assert "excursion" not in text and "rocmdash_window_above_samples" not in text
    had = _snap(True)
    had.timestamp = never.timestamp
    had.window_excursions = had.window_excursion_thresholds = None
    assert render_snapshot(had, hostname="n1") == text


def test_render_snapshot_excursion_families():
    from rocmdash.prom.exposition import parse_text, render_snapshot

    snap, plain = _snap(True), _snap()
    snap.timestamp = plain.timestamp
    text = render_snapshot(snap, hostname="n1")
    assert text.startswith(render_snapshot(plain, hostname="n1"))  # appended: nothing before them moved
    samples = parse_text(text)
    for fam, field in FAMILIES.items():
        assert f"# TYPE {fam} gauge" in text and f"# HELP {fam} " in text
        rows = [s for s in samples if s.name == fam]
        assert len(rows) == 2 * 2 * 2
        for s in rows:
            lab = s.label_dict()
            assert {"gpu_id", "metric", "threshold"} <= set(lab)
            g, si = snap.gpu_ids.index(lab["gpu_id"]), SERIES.index(lab["metric"])
            k = [repr(float(v)) for v in snap.window_excursion_thresholds[si]].index(lab["threshold"])
            assert s.value == snap.window_excursions[g, si, k, field]
    for line in text.split("\n"):  # every sample line of the five families is an integer
        if line.split("{")[0] in FAMILIES:
            assert line.rsplit(" ", 1)[1].isdigit(), line
    assert 'threshold="700.0"' in text and 'threshold="99.0"' in text


def test_page_excursion_tables():
    from rocmdash.ui.page import window_excursion_tables

    assert window_excursion_tables(_snap()) is None
    snap = _snap(True)
    tables = window_excursion_tables(snap, selected=["1"])
    assert list(tables) == ["GPU 1"] and len(tables["GPU 1"]) == 4
    row = tables["GPU 1"][1]
    assert list(row) == ["metric", "threshold", "episodes", "longest", "current", "since"]
    assert row["metric"] == SERIES[0] and row["threshold"] == 1260.0
    assert row["episodes"] == snap.window_excursions[1, 0, 1, E_EPISODES]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_excursion_kernels_have_no_scratch_fit_lds_and_keep_4_waves(tmp_path):
    """tests/test_kernel_resources.py's check for the new file, plus the register budget: at
    most 128 VGPRs (4 waves per SIMD) in every kernel, K = 4 included."""
    import re

    res = subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/csrc", "--cuda-device-only", "-c",
         os.path.join(ROOT, "csrc", "window_excursions.hip"), "-o", str(tmp_path / "k.o"),
         "-Rpass-analysis=kernel-resource-usage"],
        capture_output=True, text=True, timeout=600,
    )
    assert res.returncode == 0, res.stderr[-3000:]
    kernels, name = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|VGPRs): (\d+)", line)
        if m and name is not None:
            kernels[name][m.group(1)] = int(m.group(2))
    assert sum("excursion_stream_kernel" in k for k in kernels) == 4 and any("excursion_finalize_kernel" in k for k in kernels)
    for k, r in kernels.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0, (k, r)
        assert r.get("LDS Size [bytes/block]", 0) <= LDS_BYTES_PER_CU // 4, (k, r)  # 4 workgroups per CU
        assert 0 < r["VGPRs"] <= VGPRS_FOR_4_WAVES, (k, r)


def test_monoid_header_under_sanitizers(tmp_path):
    """tools/excursion_monoid_check.cpp - a host-only program over the header the kernels
    compile - built with AddressSanitizer and UBSan and run here."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = tmp_path / "excursion_monoid_check"
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         f"-I{ROOT}/csrc", os.path.join(ROOT, "tools", "excursion_monoid_check.cpp"), "-o", str(exe)],
        capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "ok" in run.stdout, (run.stdout[-2000:], run.stderr[-2000:])
