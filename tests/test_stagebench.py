"""tools/stagebench.py on the device: the event timing runs and gives times, and the side stream and the blockers are made once.
No assertion on the size of a time: the machine is shared."""
import importlib.util
import math
import os

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sb():
    spec = importlib.util.spec_from_file_location("stagebench", os.path.join(REPO, "tools", "stagebench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_alternate_times_device_copies(sb):
    import torch
    side = sb.side()
    assert sb.side() is side
    src = {n: torch.zeros(mib << 20, dtype=torch.uint8, device="cuda") for n, mib in (("small", 1), ("large", 4))}
    dst = {n: torch.empty_like(s) for n, s in src.items()}

    def copy(n):
        def launch():
            with torch.cuda.stream(side):
                dst[n].copy_(src[n])
        return launch

    us = sb.alternate({n: copy(n) for n in src}, 2, repeats=3, warm=1)
    side.synchronize()
    assert list(us) == ["small", "large"]
    for n, v in us.items():
        assert len(v) == 3 and all(math.isfinite(x) and x > 0 for x in v), (n, v)


def test_blockers_are_made_once(sb):
    import torch
    a = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)

    def launch():
        with torch.cuda.stream(sb.side()):
            b.copy_(a)

    sb.device_us(launch, 2)
    first = torch.cuda.memory_allocated()
    assert first >= 2 * (256 << 20)
    sb.device_us(launch, 2)
    assert torch.cuda.memory_allocated() == first
