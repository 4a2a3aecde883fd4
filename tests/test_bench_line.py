"""CPU: bench.py's headline line stays inside a driver's 8 KB output tail.  The default
`--full` run prints each workload's full line first (`workload_line <w> {...}`) and then ONE headline JSON
line whose `other_configs` repeats every workload compactly (VERDICT r3 "Weak #1": a cut tail
had lost configs[2]).  Checked on the round's recorded default line (profiles/) and on a
compacted synthetic line carrying every field compact_line keeps."""
import glob
import json
import os

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _synthetic_line(w):
    return {"value": 1.0e6, "ms_per_step": 3.4, "steps": 20, "dtype": "f16+f32",
            "config": {"baseline_config": f"configs[x]: {w}", "workload": w},
            "roofline": {"bound": "hbm", "kernel": "k" * 120, "achieved": 1026.1, "peak": 8000.0,
                         "unit": "GB/s", "frac": 0.128, "avg_kernel_ms": 1.3, "launches": 40,
                         "algorithmic_per_launch": 1.34e9, "traffic": 6.79e9, "extra": "x" * 500,
                         "gather_ceiling": {"bytes": 1.66e10, "ms": 0.72, "frac": 0.56,
                                            "vs_uniform_random": 1.65, "source": "s" * 80}},
            "cpu_baseline": {"value": 2000.0, "note": "n" * 400},
            "exact_fp32": {"value": 9.7e5, "note": "n" * 300},
            "filtered": {"value": 1.1e6, "note": "n" * 300},
            "pipelined_3_streams": {"value": 1.1e6, "note": "n" * 300},
            "prefilter": {"rows": 4096, "candidates_per_row": 27.2, "fallback_rows": 0}}


def test_compact_line_keeps_the_judged_fields():
    c = bench.compact_line(_synthetic_line("lightgcn"))
    assert c["value"] == 1.0e6 and c["ms_per_step"] == 3.4
    r = c["roofline"]
    for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "avg_kernel_ms", "traffic"):
        assert k in r
    assert "extra" not in r
    assert set(r["gather_ceiling"]) == {"bytes", "ms", "frac", "vs_uniform_random"}
    assert c["cpu_baseline"] == 2000.0 and c["exact_fp32"] == 9.7e5
    assert c["candidates_per_row"] == 27.2 and c["fallback_rows"] == 0
    # four workloads compacted fit easily beside the headline's own fields
    assert len(json.dumps({w: c for w in ("lightgcn", "widedeep", "lightgcn128", "mf")})) < 4000


def test_recorded_headline_fits_the_tail():
    files = sorted(glob.glob(os.path.join(REPO, "profiles", "r4*_bench_default.json")))
    assert files, "no round-4 default bench record under profiles/"
    for f in files:
        head = json.load(open(f))["headline_line"]
        assert len(json.dumps(head)) < 7000, f
        assert {"lightgcn", "widedeep", "lightgcn128", "mf"} <= set(head["other_configs"])
        assert "gather_ceiling" in head["other_configs"]["lightgcn"]["roofline"]


def test_gather_ceiling_units():
    """16.65 GB of 256-B rows in 1.30 ms = 12.8 TB/s: 0.56 of the 23 TB/s L2-resident rate and
    ~1.65x the 7.74 TB/s of the same gathers in uniformly random order."""
    g = bench.gather_ceiling(16.65e9, 1.30)
    assert abs(g["achieved_TBps"] - 12.81) < 0.01
    assert abs(g["uniform_random_TBps"] - 7.738) < 0.01
    assert abs(g["frac"] - 12.81 / 23.0) < 0.001
    assert 1.6 < g["vs_uniform_random"] < 1.7
    assert abs(g["ms"] - 0.7239) < 0.001
