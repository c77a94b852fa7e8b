"""bench.py contract: runs under torch.distributed.run with world=2 on CPU
(gloo) and prints one valid JSON line (the driver depends on this)."""

import json
import os
import socket
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _check_json_line(stdout: str, n_gpus: int):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert lines, f"no JSON line in output:\n{stdout[-2000:]}"
    result = json.loads(lines[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert key in result, f"missing {key}"
    assert result["n_gpus"] == n_gpus
    assert result["value"] > 0
    return result


def test_bench_single_process_cpu():
    out = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
         "--model", "test-llama", "--prompt-len", "8", "--device", "cpu"],
        cwd=REPO, capture_output=True, text=True, timeout=240,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    _check_json_line(out.stdout, 1)


def test_bench_serve_stack_single_cpu():
    out = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
         "--model", "test-llama", "--prompt-len", "8", "--device", "cpu", "--stack", "serve"],
        cwd=REPO, capture_output=True, text=True, timeout=300,
    )
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    result = _check_json_line(out.stdout, 1)
    assert result["config"]["stack"] == "serve"


@pytest.mark.parametrize("stack", ["serve", "pipeline"])
def test_bench_dump_outputs_cpu(tmp_path, stack):
    """--dump-outputs writes the last timed step's outputs as float .npy files,
    identical from run to run; --steps sets the number of timed steps; --full
    is accepted."""
    import numpy as np

    dumps = []
    for name, extra in (("a", []), ("b", ["--full"])):
        out = subprocess.run(
            [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
             "--model", "test-llama", "--prompt-len", "8", "--device", "cpu", "--stack", stack,
             "--dump-outputs", str(tmp_path / name)] + extra,
            cwd=REPO, capture_output=True, text=True, timeout=300,
        )
        assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
        result = _check_json_line(out.stdout, 1)
        assert result["steps"] == 3 and result["config"]["stack"] == stack
        files = sorted(p.name for p in (tmp_path / name).iterdir())
        assert files == ["last_logits.npy", "tokens.npy"]
        dumps.append({f[:-4]: np.load(tmp_path / name / f) for f in files})
    a, b = dumps
    for f, arr in a.items():
        assert arr.dtype in (np.float32, np.float64) and np.isfinite(arr).all()
        assert np.array_equal(arr, b[f]), f
    if stack == "serve":
        assert a["tokens"].shape == (1, 4)  # the input token + one per timed step
    assert a["last_logits"].shape[0] == 1 and a["last_logits"].ndim == 2
    assert a["tokens"][0, -1] == a["last_logits"][0].argmax()


def test_bench_serve_stack_exits_through_interpreter():
    """The serve stack joins its threads and leaves by the normal interpreter
    exit (no os._exit): exit handlers registered by whoever runs it still fire."""
    code = (
        "import atexit, runpy, sys\n"
        "atexit.register(lambda: print('EXIT-HANDLER-RAN', flush=True))\n"
        "sys.argv = ['bench.py', '--gpus', '1', '--steps', '2', '--warmup', '1', '--model', 'test-llama',\n"
        "            '--prompt-len', '8', '--device', 'cpu', '--stack', 'serve']\n"
        "runpy.run_path('bench.py', run_name='__main__')\n"
    )
    out = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    _check_json_line(out.stdout, 1)
    assert out.stdout.rstrip().endswith("EXIT-HANDLER-RAN"), out.stdout[-500:]


def test_bench_serve_stack_two_rank_cpu():
    port = _free_port()
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
         "--master-addr", "127.0.0.1", "--master-port", str(port),
         "bench.py", "--gpus", "2", "--steps", "3", "--warmup", "1",
         "--model", "test-llama", "--prompt-len", "8", "--device", "cpu", "--stack", "serve"],
        cwd=REPO, capture_output=True, text=True, timeout=420,
    )
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    result = _check_json_line(out.stdout, 2)
    assert result["config"]["parallelism"] == "swarm-pp2"


def test_bench_two_rank_pipeline_cpu():
    port = _free_port()
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
         "--master-addr", "127.0.0.1", "--master-port", str(port),
         "bench.py", "--gpus", "2", "--steps", "3", "--warmup", "1",
         "--model", "test-llama", "--prompt-len", "8", "--device", "cpu", "--stack", "pipeline"],
        cwd=REPO, capture_output=True, text=True, timeout=300,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    result = _check_json_line(out.stdout, 2)
    assert result["config"]["parallelism"] == "pp2"
