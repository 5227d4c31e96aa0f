"""The child runner the five active probes share (probe/_active.py),
through each probe's own ``run_<probe>_subprocess`` binding.  No child
is started: ``subprocess.run`` is replaced in the shared module."""

import importlib
import json
import os
import subprocess
import sys

import pytest

from kubegpu_amd.probe import _active

# probe -> the size flag its binding must pass
SIZE_FLAGS = {
    "memcheck": "--bytes",
    "cucheck": "--rounds",
    "mxcheck": "--rounds",
    "fpcheck": "--rounds",
    "hostlink": "--bytes",
}


def test_the_table_covers_every_active_probe():
    assert tuple(SIZE_FLAGS) == _active.ACTIVE_PROBES


class FakeRun:
    """Records how subprocess.run was called and returns a canned
    CompletedProcess."""

    def __init__(self, stdout="", stderr="", returncode=0):
        self.stdout, self.stderr, self.returncode = stdout, stderr, returncode
        self.calls = []

    def __call__(self, cmd, **kw):
        self.calls.append((list(cmd), kw, _active._child_lock.locked()))
        return subprocess.CompletedProcess(cmd, self.returncode, self.stdout, self.stderr)


def _runner(probe):
    mod = importlib.import_module(f"kubegpu_amd.probe.{probe}")
    assert mod._child_lock is _active._child_lock  # one lock for all five
    return getattr(mod, f"run_{probe}_subprocess")


@pytest.mark.parametrize("probe", _active.ACTIVE_PROBES)
def test_child_command_environment_lock_and_parsing(probe, monkeypatch):
    run = _runner(probe)
    root = _active._REPO_ROOT
    assert os.path.isdir(os.path.join(root, "kubegpu_amd", "probe"))

    # the record is the last stdout line; the child's exit code is added
    fake = FakeRun(stdout='warning: noise\n{"ok": false, "n": 7}\n', returncode=1)
    monkeypatch.setattr(_active.subprocess, "run", fake)
    monkeypatch.delenv("PYTHONPATH", raising=False)
    assert run(3, 4096, timeout_s=7.5) == {"ok": False, "n": 7, "exit_code": 1}
    cmd, kw, locked = fake.calls[0]
    assert cmd == [sys.executable, "-m", f"kubegpu_amd.probe.{probe}",
                   "--device", "3", SIZE_FLAGS[probe], "4096"]
    assert locked and not _active._child_lock.locked()
    assert kw["timeout"] == 7.5 and kw["capture_output"] is True and kw["text"] is True
    assert kw["env"]["PYTHONPATH"] == root

    # a PYTHONPATH that was set is kept, behind the repository root
    monkeypatch.setenv("PYTHONPATH", "/somewhere/else")
    run(0, 16)
    cmd, kw, locked = fake.calls[1]
    assert cmd[-4:] == ["--device", "0", SIZE_FLAGS[probe], "16"] and locked
    assert kw["env"]["PYTHONPATH"] == root + os.pathsep + "/somewhere/else"
    assert os.environ["PYTHONPATH"] == "/somewhere/else"  # the parent's is untouched


@pytest.mark.parametrize("probe", _active.ACTIVE_PROBES)
@pytest.mark.parametrize("stdout", ["", "\n\n", "Traceback (most recent call last):\nboom\n"])
def test_child_without_json_could_not_run(probe, stdout, monkeypatch):
    fake = FakeRun(stdout=stdout, stderr="x" * 600 + "the end", returncode=0)
    monkeypatch.setattr(_active.subprocess, "run", fake)
    rec = _runner(probe)(1, 32)
    assert rec["exit_code"] == _active.EXIT_CANNOT_RUN == 2
    assert rec["error"].startswith(f"no JSON from {probe} child: ")
    assert rec["error"].endswith("the end")  # the tail of stderr, 500 characters
    assert len(rec["error"]) == len(f"no JSON from {probe} child: ") + 500
    assert set(rec) == {"error", "exit_code"}
    assert json.loads(json.dumps(rec)) == rec
