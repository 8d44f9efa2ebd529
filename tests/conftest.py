import os
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
# block journal at test scale: 32 MiB segments, not zero-filled (every store and chunkserver
# the tests start would otherwise write 512 MiB of spare segments); larger blocks take the
# per-file path, which the tests exercise as well
os.environ.setdefault("DFS_JOURNAL_SEG_MB", "32")
os.environ.setdefault("DFS_JOURNAL_ZERO_FILL", "0")
os.environ.setdefault("DFS_JOURNAL_PARTS", "4")  # 8 MiB part files at test scale


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (HIP device)")
    config.addinivalue_line("markers", "slow: multi-process cluster test")


@pytest.fixture(scope="session")
def native():
    from rust_hadoop_generated_by_llm_amd import native as n

    return n.lib


@pytest.fixture(scope="session")
def has_gpu():
    from rust_hadoop_generated_by_llm_amd import native as n

    return n.gpu_count() > 0


@pytest.fixture(scope="session")
def can_pin_existing_memory(native, has_gpu, tmp_path_factory):
    """Whether the GPU runtime can pin memory that was not allocated pinned, such as another
    process's shared-memory arena (some hosts refuse it). Probed once with a small buffer."""
    if not has_gpu:
        return False
    import numpy as np

    store = native.ChunkStore(str(tmp_path_factory.mktemp("pinprobe")), "", 0, 64 << 20, 0, 100, 2, 1, False)
    buf = np.zeros(1 << 16, dtype=np.uint8)
    ok = bool(store.register_host(buf))
    if ok:
        store.unregister_host(buf)
    del store
    return ok
