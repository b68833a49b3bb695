"""The harness with --csr-on-device (spmv-samples_amd/host/main.cpp): the stored entries are uploaded and the device
builds Ap / Aj / Ax (mi355_spmv_coo_to_csr, or mi355_spmv_coo_to_csr_symmetric for a symmetric file).  The CPU check
still runs on the host-made CSR, so the "Compute delta" table must be the one the host path prints."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT

EXE = os.path.join(ROOT, "spmv-samples_amd", "bin", "spmv")
KINDS = ["hip_vector", "hip_merge", "hip_light"]


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "spmv-samples_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "spmv-samples_amd", "host")], check=True)
    return EXE


def run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)


def head_and_delta_table(out):
    """Everything up to and including the "Compute delta" table (the dataset lines, then one line per kind)."""
    assert "Compute delta:\n" in out and "\nTime cost:\n" in out, out
    head = out[:out.index("\nTime cost:\n")]
    assert head.count("] sum: ") == len(KINDS), out
    return head


def test_usage_names_the_switch_on_a_further_line(exe):
    r = run(exe)
    lines = r.stderr.splitlines()
    assert r.returncode == 1 and lines[0] == "usage: ./bin/<program-name>  <filename.mtx>  <SpMV_kind_string>..."
    assert any("--csr-on-device" in l for l in lines[1:])
    r = run(exe, "synthetic:band:n=1000,k=4,w=8", "hip_vector", "--csr-on-device")
    assert r.returncode == 1 and "needs a Matrix Market file" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--dtype", "f64", "--offset", "64"]])
def test_symmetric_fixture_gives_the_same_delta_table(exe, extra):
    path = os.path.join(GOLD, "c1_1138_bus_standin.mtx")
    host = run(exe, path, *KINDS, "--iters", "5", *extra)
    dev = run(exe, path, *KINDS, "--iters", "5", *extra, "--csr-on-device")
    assert host.returncode == 0 and dev.returncode == 0, host.stderr + dev.stderr
    assert "n_rows: 1138  n_cols: 1138  nnz: 4054" in dev.stdout
    assert head_and_delta_table(dev.stdout) == head_and_delta_table(host.stdout)
    assert "nan" not in head_and_delta_table(dev.stdout)


@pytest.mark.gpu
def test_general_file_gives_the_same_delta_table(exe, tmp_path):
    rng = np.random.RandomState(3)
    n, nnz = 20000, 300000
    r, c = rng.randint(0, n, nnz), rng.randint(0, n + 50, nnz)
    v = rng.uniform(-1, 1, nnz)
    path = tmp_path / "general.mtx"
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (n, n + 50, nnz))
        np.savetxt(f, np.stack([r + 1, c + 1, v], 1), fmt="%d %d %.9g")
    host = run(exe, str(path), *KINDS, "--iters", "5")
    dev = run(exe, str(path), *KINDS, "--iters", "5", "--csr-on-device")
    assert host.returncode == 0 and dev.returncode == 0, host.stderr + dev.stderr
    assert "n_rows: 20000  n_cols: 20050  nnz: 300000" in dev.stdout
    assert head_and_delta_table(dev.stdout) == head_and_delta_table(host.stdout)
    assert "nan" not in head_and_delta_table(dev.stdout)
