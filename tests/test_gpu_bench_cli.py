"""bench.py's plain run on the GPU: ``--steps`` timed steps, the headline line
alone (nothing of ``--full``), and ``--dump-outputs`` writing the last step's
acquisition values and their maximum as fp64 ``.npy``."""
import json
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_plain_run_headline_and_dump(tmp_path, monkeypatch, capsys):
    import bench
    out = tmp_path / "dump"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1",
                                      "--dump-outputs", str(out)])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "BO_BENCH_REHEARSE"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "acq-evals/s" and line["dtype"] == "f64" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0
    # value is q x restarts x MC evaluations per second of the timed steps
    assert line["value"] == pytest.approx(16 * 512 * 512 / (1e-3 * line["ms_per_step"]), rel=1e-9)
    for k in ("roofline", "cholesky", "gp_fit", "other_configs", "cpu_baseline", "fwd_bwd", "check"):
        assert k not in line
    acq, best = np.load(out / "acq.npy"), np.load(out / "best.npy")
    assert acq.dtype == np.float64 and acq.shape == (bench.RESTARTS,)
    assert best.dtype == np.float64 and best.shape == (1,)
    assert np.isfinite(acq).all() and (acq >= 0).all() and (acq > 0).any()
    assert best[0] == acq.max()
