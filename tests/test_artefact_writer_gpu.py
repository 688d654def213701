"""Native dataset persister on the GPU: files are byte for byte what
``np.save(y)`` followed by ``np.save(X)`` writes, slots are reused safely,
source tensors may die right after ``submit``, a failing destination
surfaces as a Python exception and leaves the persister working, and the
whole cycle persists the same bytes through the native and the Python
path."""
import io
import os
from datetime import date, timedelta

import numpy as np
import pytest
import torch

from bodywork_mlops_demo_amd import ops
from bodywork_mlops_demo_amd.pipeline.cycle import CycleState, run_cycle
from bodywork_mlops_demo_amd.store import LocalStore, contract

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [1, 3, 255, 257, 65_537, 1_000_003, 1]  # 7 files through 3 slots


def _want_bytes(y: np.ndarray, X: np.ndarray) -> bytes:
    bio = io.BytesIO()
    np.save(bio, y)
    np.save(bio, X)
    return bio.getvalue()


def _day(n: int, seed: int):
    g = torch.Generator(device="cpu").manual_seed(seed)
    y = torch.randn(n, generator=g, dtype=torch.float32)
    X = torch.rand(n, generator=g, dtype=torch.float32) * 100.0
    return y, X


def _read(path) -> bytes:
    with open(path, "rb") as f:
        return f.read()


def test_files_equal_np_save_with_slot_reuse(tmp_path):
    p = ops.dataset_persister(2, 3)
    assert (p.workers, p.slots) == (2, 3)
    want, handles = {}, []
    for i, n in enumerate(SIZES):
        y, X = _day(n, i)
        path = str(tmp_path / f"day-{i}.npy")
        want[path] = _want_bytes(y.numpy(), X.numpy())
        handles.append(p.submit(y.to(DEV), X.to(DEV), path))
    p.drain()
    assert all(h.done() for h in handles)
    for h in handles:
        h.result()  # raises if the job failed
        t = h.timings()
        assert set(t) == {"slot_wait_s", "ready_s", "write_s", "rename_s"}
        assert all(v >= 0.0 for v in t.values())
    for path, raw in want.items():
        assert _read(path) == raw, path
    assert sorted(os.listdir(tmp_path)) == sorted(
        os.path.basename(k) for k in want)  # no temporaries left
    p.close()


def test_sources_may_die_right_after_submit(tmp_path):
    """The recordStream contract: the allocator must not hand the source
    blocks to new compute-stream tensors while the side-stream copy is
    still reading them."""
    p = ops.dataset_persister(2, 3)
    n = 1_000_003
    want = {}
    for i in range(4):
        y, X = _day(n, 100 + i)
        path = str(tmp_path / f"day-{i}.npy")
        want[path] = _want_bytes(y.numpy(), X.numpy())
        y_d, X_d = y.to(DEV), X.to(DEV)
        p.submit(y_d, X_d, path)
        del y_d, X_d
        # same-sized allocations on the compute stream, filled at once
        a = torch.full((n,), -1.0, device=DEV)
        b = torch.full((n,), -2.0, device=DEV)
        del a, b
    p.drain()
    for path, raw in want.items():
        assert _read(path) == raw, path
    p.close()


def test_failing_destination_raises_and_persister_goes_on(tmp_path):
    p = ops.dataset_persister(2, 3)
    blocker = tmp_path / "a-file"
    blocker.write_bytes(b"x")
    y, X = _day(257, 7)
    bad = p.submit(y.to(DEV), X.to(DEV), str(blocker / "day.npy"))
    with pytest.raises(RuntimeError, match="day.npy"):
        p.drain()
    assert bad.done()
    with pytest.raises(RuntimeError):
        bad.result()
    # reported once; afterwards the persister works as before
    p.drain()
    good = str(tmp_path / "good.npy")
    p.submit(y.to(DEV), X.to(DEV), good).result()
    assert _read(good) == _want_bytes(y.numpy(), X.numpy())

    # without a drain the error surfaces at the next submit on that slot
    q = ops.dataset_persister(1, 1)
    q.submit(y.to(DEV), X.to(DEV), str(blocker / "again.npy"))
    with pytest.raises(RuntimeError, match="again.npy"):
        q.submit(y.to(DEV), X.to(DEV), str(tmp_path / "never.npy"))
    after = str(tmp_path / "after.npy")
    q.submit(y.to(DEV), X.to(DEV), after)
    q.drain()
    assert _read(after) == _want_bytes(y.numpy(), X.numpy())
    assert not (tmp_path / "never.npy").exists()
    assert not [f for f in os.listdir(tmp_path) if f.startswith(".tmp-")]
    p.close()
    q.close()


def test_submit_rejects_what_it_cannot_write(tmp_path):
    p = ops.dataset_persister(1, 2)
    y, X = _day(16, 3)
    path = str(tmp_path / "d.npy")
    with pytest.raises(RuntimeError):
        p.submit(y, X, path)  # CPU tensors
    with pytest.raises(RuntimeError):
        p.submit(y.to(DEV).double(), X.to(DEV).double(), path)
    with pytest.raises(RuntimeError):
        p.submit(y.to(DEV)[::2], X.to(DEV)[::2], path)  # not contiguous
    p.drain()
    assert os.listdir(tmp_path) == []
    p.close()


class _OtherLocalStore(LocalStore):
    """Not a plain LocalStore: CycleState must take the Python path."""


def _run_cycles(store, n_rows=1000, n_cycles=4):
    start = date(2026, 1, 1)
    state = CycleState(DEV, start, history_days=1)
    cache: dict = {}
    per_day = {}
    for _ in range(n_cycles):
        cap: dict = {}
        run_cycle(state, store, n_rows, model_type="linear",
                  persist_fmt="npy", scorer_cache=cache, capture=cap)
        per_day[state.date] = (cap["labels"].cpu().numpy(),
                               cap["X"].cpu().numpy())
    state.drain_io()
    y0, X0 = ops.datagen(n_rows, start.timetuple().tm_yday,
                         start.toordinal() * 1000, device=DEV)
    per_day[start] = (y0.cpu().numpy(), X0.cpu().numpy())
    return state, per_day


def test_whole_cycle_native_and_python_paths_write_the_same(tmp_path):
    n_cycles = 4
    native = LocalStore(str(tmp_path / "native"))
    state, per_day = _run_cycles(native, n_cycles=n_cycles)
    # what test_gpu_cycles_persist_every_day_exactly expects
    assert getattr(state, "_persister", None) is not None
    assert state._io_futures == []
    assert all(f.done() for f in state._pin_futures.values())
    start = date(2026, 1, 1)
    assert sorted(per_day) == [start + timedelta(days=i)
                               for i in range(n_cycles + 1)]
    assert len(native.list_keys(contract.DATASETS_PREFIX)) == n_cycles + 1
    for d, (y, X) in per_day.items():
        key = contract.dataset_key(d, "npy")
        got_y, got_X = native.get_dataset(key)
        assert np.array_equal(got_y, y) and np.array_equal(got_X, X), d
        assert native.get_bytes(key) == _want_bytes(y, X), d
    last = per_day[state.date]
    assert np.array_equal(state.y.cpu().numpy(), last[0])
    assert np.array_equal(state.X.cpu().numpy(), last[1])

    other = _OtherLocalStore(str(tmp_path / "python"))
    state2, per_day2 = _run_cycles(other, n_cycles=n_cycles)
    assert getattr(state2, "_persister", None) is None  # Python path
    assert all(f.done() for f in state2._pin_futures.values())
    keys = native.list_keys(contract.DATASETS_PREFIX)
    assert other.list_keys(contract.DATASETS_PREFIX) == keys
    for key in keys:
        assert other.get_bytes(key) == native.get_bytes(key), key
