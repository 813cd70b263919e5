"""Host side of fused.render_fused_eval_views (no GPU): the chunk plan that keeps a batch of
views inside the stacked binning's limits, and the argument checks, which come before any
device work (so they raise ValueError here, where the scene is on the CPU)."""
import pytest
import torch

from gaussctrl_exp_amd import fused
from gaussctrl_exp_amd.camera import synthetic_camera
from gaussctrl_exp_amd.fused import _plan_view_chunks, render_fused_eval_views
from gaussctrl_exp_amd.scene import synthetic_scene

INT_MAX = 2 ** 31 - 1


def _ok(chunks, n, tby, views, max_points, tbx=1):
    assert sum(chunks) == views and min(chunks) >= 1
    assert max(chunks) - min(chunks) <= 1
    for c in chunks:
        assert c * tby <= 65535 and c * n <= INT_MAX and c * n <= max_points
        assert tbx * c * tby <= INT_MAX


def test_small_batch_is_one_chunk():
    assert _plan_view_chunks(300000, 32, 8) == [8]
    assert _plan_view_chunks(300000, 32, 1) == [1]
    assert _plan_view_chunks(0, 32, 5) == [5]


def test_row_field_limit_splits():
    # 68 tile rows per view (1080 px): 963 views fill the 16-bit row field, 964 do not
    assert _plan_view_chunks(10, 68, 963, max_points=10 ** 9) == [963]
    chunks = _plan_view_chunks(10, 68, 964, max_points=10 ** 9)
    assert chunks == [482, 482]
    _ok(chunks, 10, 68, 964, 10 ** 9)
    # a view as tall as the field itself: one view per chunk
    assert _plan_view_chunks(10, 65535, 3, max_points=10 ** 9) == [1, 1, 1]


def test_int_limit_splits():
    n = 300_000_000  # 8 views = 2.4e9 virtual points > INT32_MAX
    chunks = _plan_view_chunks(n, 4, 8, max_points=10 ** 12)
    assert chunks == [4, 4]  # INT_MAX // n = 7 views at most; balanced
    _ok(chunks, n, 4, 8, 10 ** 12)
    # the stacked tile count must fit int as well
    chunks = _plan_view_chunks(10, 4096, 16, max_points=10 ** 9, tbx=65535)
    _ok(chunks, 10, 4096, 16, 10 ** 9, tbx=65535)
    assert len(chunks) > 1


def test_max_points_splits_and_sums():
    assert _plan_view_chunks(3000, 9, 3, max_points=6000) == [2, 1]
    assert _plan_view_chunks(3000, 9, 3, max_points=3000) == [1, 1, 1]
    assert _plan_view_chunks(3000, 9, 7, max_points=3 * 3000 + 2999) == [3, 2, 2]
    for views in range(1, 40):
        for mp in (1000, 2500, 7000, 10 ** 6):
            _ok(_plan_view_chunks(1000, 9, views, max_points=mp), 1000, 9, views, mp)
    # the default bound: 16 views of a 1M scene in one chunk, 17 in two
    assert fused.VIEWS_MAX_POINTS == 1 << 24
    assert _plan_view_chunks(1 << 20, 68, 16) == [16]
    assert _plan_view_chunks(1 << 20, 68, 17) == [9, 8]


def test_plan_errors():
    with pytest.raises(ValueError):
        _plan_view_chunks(3000, 9, 3, max_points=2999)  # max_points < N
    with pytest.raises(ValueError):
        _plan_view_chunks(3000, 9, 0)
    with pytest.raises(ValueError):
        _plan_view_chunks(3000, 65536, 1)  # one view alone overflows the row field


@pytest.fixture(scope="module")
def scene():
    return synthetic_scene(50, 3, seed=1)


def test_argument_errors_come_before_device_work(scene):
    cam = synthetic_camera(64, 48)
    bg = torch.zeros(3)
    with pytest.raises(ValueError, match="no cameras"):
        render_fused_eval_views(scene, [], 3, bg)
    with pytest.raises(ValueError, match="share one"):
        render_fused_eval_views(scene, [cam, synthetic_camera(64, 64)], 3, bg)
    for bad in (torch.zeros(4), torch.zeros(3, 3), torch.zeros(2, 3, 1), [0.0, 0.0, 0.0]):
        with pytest.raises(ValueError, match="background"):
            render_fused_eval_views(scene, [cam, cam], 3, bad)
    for deg in (-1, 4):
        with pytest.raises(ValueError, match="degree"):
            render_fused_eval_views(scene, [cam], deg, bg)
    with pytest.raises(ValueError, match="max_points"):
        render_fused_eval_views(scene, [cam], 3, bg, max_points=49)


def test_valid_arguments_on_the_cpu_reach_the_device_check(scene):
    """Nothing runs on the CPU: valid arguments get as far as the library's device check."""
    with pytest.raises(RuntimeError, match="ROCm device"):
        render_fused_eval_views(scene, [synthetic_camera(64, 48)], 3, torch.zeros(3))
