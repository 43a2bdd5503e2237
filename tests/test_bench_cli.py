"""bench.py's command line: --steps / --warmup, --full (secondary figures) and --dump-outputs.  CPU only."""
import importlib.util
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("clrrt_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_options(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.no_cpu and a.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()
    # the dump stays under 64 MB: 8 float64 fields (19 values) + 2 float32 per node
    assert bench.DUMP_NODES * (19 * 8 + 2 * 4) <= 64 << 20
