"""bench.py's command line (CPU side): a plain run is the default, and what belongs to --full is not accepted without it."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_plain_run_is_the_default():
    args = _bench().parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert args.full is False and (args.steps, args.warmup, args.gpus) == (20, 5, 1)
    assert _bench().parse_args(["--full"]).full is True


def test_with_c5_needs_full():
    bench = _bench()
    with pytest.raises(SystemExit):
        bench.parse_args(["--gpus", "2", "--with-c5"])
    assert bench.parse_args(["--gpus", "2", "--with-c5", "--full"]).with_c5 is True
