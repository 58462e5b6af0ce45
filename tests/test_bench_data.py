"""bench.py's data set: Generator.chunks draws the chunks on several threads, and the array it returns is the chunks'
own streams laid end to end, whatever the number of threads and however the last chunk is cut."""
import numpy as np

import bench


def test_chunks_are_the_streams_laid_end_to_end(monkeypatch):
    gen = bench.Generator(d=48, latent=8, n_comp=64)
    want = np.concatenate([gen.rows(1000, stream=0), gen.rows(1000, stream=1), gen.rows(300, stream=2)])
    for cpus in (1, 5):
        monkeypatch.setattr(bench, "usable_cpus", lambda: cpus)
        got = gen.chunks(2300, 1000)
        assert got.dtype == np.float32 and got.flags.c_contiguous and np.array_equal(got, want), cpus
