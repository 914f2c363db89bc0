"""`--sampler reference` (native host code, macr_amd/host_sampler.py) against `--sampler python` (the reference's loop) through
the CLIs on the GPU: the same batches reach the same kernels, so the printed lines are the same; and the device side of
ReferenceStreamSampler -- one pass buffer, views, the host view that travels with every batch."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import REPO, dataset_args

pytestmark = pytest.mark.gpu

_TIMES = re.compile(r"\[\d+\.\ds(?: \+ \d+\.\ds)?\]")          # wall-clock brackets of the log lines: "[0.3s + 0.1s]"


def _run_cli(cmd, cwd):
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    out = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout


def _report_lines(out, heads):
    """the loss and metric lines of a run, wall-clock brackets removed"""
    return [_TIMES.sub("[]", l) for l in out.splitlines() if l.startswith(heads)]


def test_mf_cli_prints_the_same_lines_under_reference_and_python(tmp_path):
    os.symlink(os.path.join(REPO, "data"), tmp_path / "data")
    common = [os.path.join(REPO, "macr_mf", "train.py"), "--dataset", "addressa", "--batch_size", "1024", "--cuda", "0",
              "--epoch", "2", "--log_interval", "1", "--save_flag", "0"]
    ref = _report_lines(_run_cli(common + ["--sampler", "reference"], str(tmp_path)), ("Epoch ",))
    py = _report_lines(_run_cli(common + ["--sampler", "python"], str(tmp_path)), ("Epoch ",))
    print("\n".join(ref + py))
    assert len(py) == 2 and all("train==[" in l and "recall=[" in l for l in py), py
    assert ref == py


def test_lightgcn_cli_prints_the_same_lines_under_reference_and_python(tmp_path):
    """--loss bceboth --test rubiboth at --log_interval 1: every epoch runs the test-loss pass too (sample_test batches), and
    the second epoch's batches depend on the states both passes of the first one left"""
    common = [os.path.join(REPO, "macr_lightgcn", "LightGCN.py"), "--data_path", os.path.join(REPO, "data") + "/",
              "--dataset", "addressa", "--batch_size", "1024", "--gpu_id", "0", "--layer_size", "[64,64]", "--Ks", "[20]",
              "--loss", "bceboth", "--test", "rubiboth", "--c", "40", "--alpha", "1e-2", "--beta", "1e-3", "--verbose", "1",
              "--epoch", "2", "--log_interval", "1", "--save_flag", "0"]
    ref = _report_lines(_run_cli(common + ["--sampler", "reference"], str(tmp_path)), ("Epoch ", "c:"))
    py = _report_lines(_run_cli(common + ["--sampler", "python"], str(tmp_path)), ("Epoch ", "c:"))
    print("\n".join(ref + py))
    assert len(py) == 4 and sum(l.startswith("c:40.00 recall=[") for l in py) == 2, py
    assert ref == py


def test_mf_cli_resume_under_reference_continues_the_python_run(tmp_path):
    """2 epochs + `--resume 1` for 2 more under `reference` = 4 epochs straight under `python`, on the final epoch's line: the
    checkpointed `random` / numpy states are those the Python loop would have left"""
    os.symlink(os.path.join(REPO, "data"), tmp_path / "data")
    common = [os.path.join(REPO, "macr_mf", "train.py"), "--dataset", "addressa", "--batch_size", "1024", "--cuda", "0",
              "--log_interval", "1"]
    straight = _run_cli(common + ["--saveID", "py", "--save_flag", "0", "--epoch", "4", "--sampler", "python"], str(tmp_path))
    _run_cli(common + ["--saveID", "ref", "--epoch", "2", "--sampler", "reference"], str(tmp_path))
    resumed = _run_cli(common + ["--saveID", "ref", "--epoch", "4", "--resume", "1", "--sampler", "reference"], str(tmp_path))
    assert "resumed from epoch 1" in resumed
    want, got = _report_lines(straight, ("Epoch 3 ",)), _report_lines(resumed, ("Epoch 3 ",))
    print("\n".join(want + got))
    assert len(want) == 1 and got == want


def test_device_views_of_a_pass_equal_the_host_chunk():
    from macr_amd.data import MFData
    from macr_amd.host_sampler import ReferenceStreamSampler
    data = MFData(dataset_args("addressa"))
    dev = torch.device("cuda", 0)
    n = 23
    random.seed(3)
    np.random.seed(3)
    want = ReferenceStreamSampler.for_mf(data).generate(n)
    after = random.getstate()
    for chunk in (None, 5):                                  # one upload, and several through the two pinned buffers
        random.seed(3)
        np.random.seed(3)
        s = ReferenceStreamSampler.for_mf(data, device=dev, chunk_batches=chunk)
        s.begin_pass(n)
        assert random.getstate() == after                    # the live state has moved on by the whole pass already
        for k in range(n):
            b = s.sample()
            assert b.device.type == "cuda" and b.dtype == torch.int32 and tuple(b.shape) == (3, 1024) and b.is_contiguous()
            assert isinstance(b._macr_host_batch, np.ndarray) and b._macr_host_batch.shape == tuple(b.shape)
            assert np.array_equal(b._macr_host_batch, want[k])
            assert np.array_equal(b.cpu().numpy(), b._macr_host_batch)
        with pytest.raises(RuntimeError):
            s.sample()
        s.begin_pass(2)                                      # the next pass reuses the buffers
        assert np.array_equal(s.sample().cpu().numpy(), s._host[0])
