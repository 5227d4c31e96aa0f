import os
import pathlib
import shutil
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pytest_configure(config):
    config.addinivalue_line(
        "markers", "gpu: test requires a real MI355X GPU (run via gpurun)"
    )


@pytest.fixture
def sock_dir():
    """Short directory for AF_UNIX sockets.

    sun_path holds at most 107 bytes and gRPC refuses longer paths, which a
    pytest tmp_path under a deep home or TMPDIR exceeds.
    """
    base = "/tmp" if os.access("/tmp", os.W_OK | os.X_OK) else None
    d = tempfile.mkdtemp(prefix="kg-", dir=base)
    yield pathlib.Path(d)
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture
def fixture_8x():
    from kubegpu_amd.discovery import fixtures

    return fixtures.fixture_8x_mi355x()


@pytest.fixture
def fixture_2hive():
    from kubegpu_amd.discovery import fixtures

    return fixtures.fixture_2hive_8gpu()


@pytest.fixture
def fixture_no_xgmi():
    from kubegpu_amd.discovery import fixtures

    return fixtures.fixture_4x_no_xgmi()
