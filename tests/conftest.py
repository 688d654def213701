import os
import sys

import pytest
import torch

# The suite imports the package from the source tree (nothing is installed),
# starts child interpreters that import it too, and uses repo-relative paths
# (pipeline.yaml, tools/...).  Make that hold however pytest was launched:
# `pytest`, `python -m pytest`, from the repo root or from elsewhere.
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
os.environ["PYTHONPATH"] = os.pathsep.join(
    p for p in (REPO, os.environ.get("PYTHONPATH")) if p)


@pytest.fixture(autouse=True)
def _run_from_repo_root(monkeypatch):
    monkeypatch.chdir(REPO)


def pytest_configure(config):
    config.addinivalue_line(
        "markers", "gpu: needs a ROCm GPU (run on an MI355X box)"
    )


def pytest_collection_modifyitems(config, items):
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU available")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)


@pytest.fixture()
def tmp_store(tmp_path):
    from bodywork_mlops_demo_amd.store import LocalStore

    return LocalStore(str(tmp_path / "store"))
