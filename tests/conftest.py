import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu)")


@pytest.fixture(scope="session")
def oracle():
    """CPU oracle (test infrastructure) -- builds oracle/libzkm_oracle.so with gcc if needed."""
    from oracle.oracle_py import Oracle
    return Oracle()


@pytest.fixture(scope="session")
def zkm():
    import zkm_amd
    zkm_amd.load()
    return zkm_amd


@pytest.fixture(scope="session")
def ctx(zkm):
    """GPU context; fails loudly (no CPU fallback) if the extension or the GPU is missing."""
    c = zkm.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="session")
def oracle_proof_2_20(oracle):
    """The CPU oracle's proof of the bench workload (PoseidonStark 262 x 2^20, witness seed 100 = segment 0 of bench.py / BASELINE
    configs 2 and 3), computed ONCE per session (about a minute on 64 host threads, ~30 GB of host memory) and shared by the tests
    that compare GPU proofs with it.  A dict: trace xor-checksum and sampled words, the proof words, the oracle's wall and stage seconds."""
    import time
    import numpy as np
    if (os.cpu_count() or 1) < 32:
        # ~70 s on 64 threads; on a small host it would eat the GPU suite's time limit and every later test with it.  The tests that use
        # this fixture keep their size-independent checks (oracle verifier, single-context equality) and skip the word-for-word part.
        return None
    log_n = 20
    n = 1 << log_n
    old = oracle.get_threads()
    from bench import cpu_quota
    threads = max(1, min(64, os.cpu_count() or 1, cpu_quota() or 64))      # (the GPU boxes grant 16 CPUs of the 256 they show)
    oracle.set_threads(threads)
    # (all 256 cores for the row-parallel stages were measured in r04_a: 94.6 s against 72.6 s on 64 threads -- the leaf gather is
    # memory-latency bound; profiles/cpu_oracle_full_size.json "all_cores")
    try:
        trace = oracle.poseidon_trace(100, n, log_n)
        aux = np.zeros(4 * n, dtype=np.uint64)
        t0 = time.time()
        proof, stages = oracle.prove(trace, log_n, aux, [1, 1], want_stages=True)
        secs = time.time() - t0
    finally:
        oracle.set_threads(old)
    out = {"xor": int(np.bitwise_xor.reduce(trace)), "sample": trace[::4099].copy(), "proof": proof, "seconds": secs, "stage_s": stages,
           "threads": threads, "wide_threads": None, "cpu_quota": cpu_quota()}
    del trace
    return out
