"""bench.py --dump-outputs: the arrays hold every Goldilocks element exactly, the trace sample is the same from run to run,
and at the default shape the files stay far below 64 MB."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bench)


class _Buf:
    def __init__(self, a):
        self.a = a

    def download(self):
        return self.a.reshape(-1).copy()


def _whole(h):
    return h[..., 0].astype(np.uint64) | (h[..., 1].astype(np.uint64) << np.uint64(32))


def test_dump_outputs_exact_and_deterministic(tmp_path):
    k, n = 5, 1 << 12
    trace = bench.splitmix64_felts(3, k * n)
    cap = bench.splitmix64_felts(4, 4 << bench.CAP_H)
    cap[:4] = [0, 0xFFFFFFFF, 1 << 32, 0xFFFFFFFF00000000]   # the edges of the two 32-bit halves (the cap is written whole)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), _Buf(trace), _Buf(cap), k, n)
    got_cap = np.load(tmp_path / "a" / "merkle_cap.npy")
    got = np.load(tmp_path / "a" / "trace_sample.npy")
    assert got_cap.dtype == got.dtype == np.float64
    assert (_whole(got_cap).reshape(-1) == cap).all()
    idx = np.unique(np.random.default_rng(bench.SEED).integers(0, k * n, size=min(bench.DUMP_SAMPLE, k * n), dtype=np.int64))
    assert (_whole(got) == trace[idx]).all()
    assert (got == np.load(tmp_path / "b" / "trace_sample.npy")).all()


def test_dump_outputs_size_bound_at_the_default_shape():
    sample_bytes = min(bench.DUMP_SAMPLE, bench.COLS << bench.LOG_N) * 2 * 8
    cap_bytes = (1 << bench.CAP_H) * 4 * 2 * 8
    assert sample_bytes + cap_bytes <= 64 << 20
