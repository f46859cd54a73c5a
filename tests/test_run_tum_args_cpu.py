"""tools/run_tum.py without a GPU: the camera of a pyramid level (Camera::Scaled, LV/camera.h:1696-1705, in the pixel-corner
convention) and the three input-conditioning options of the command line."""
import pytest

from tools import run_tum


def test_level_1_camera_of_a_640x480_dataset():
    cam = run_tum.scaled_camera([525.0, 525.0, 319.5, 239.5], 640, 480, 1)
    assert (cam.width, cam.height) == (320, 240)
    assert (cam.fx, cam.fy, cam.cx, cam.cy) == (262.5, 262.5, 159.75, 119.75)


def test_level_0_is_the_dataset_camera_and_sizes_round_half_up():
    cam = run_tum.scaled_camera([525.0, 520.0, 319.5, 239.5], 640, 480, 0)
    assert (cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height) == (525.0, 520.0, 319.5, 239.5, 640, 480)
    cam = run_tum.scaled_camera([500.0, 500.0, 100.0, 100.0], 642, 481, 2)      # int(0.25 * 642 + 0.5), int(0.25 * 481 + 0.5)
    assert (cam.width, cam.height) == (161, 120) and cam.fx == 125.0 and cam.cx == 25.0


def test_command_line_options():
    a = run_tum.arg_parser().parse_args(["dir"])
    assert (a.pyramid_level_for_depth, a.pyramid_level_for_color, a.median_filter_and_densify_iterations) == (0, 0, 0)
    a = run_tum.arg_parser().parse_args(["dir", "--pyramid-level-for-depth", "1", "--pyramid-level-for-color", "2",
                                         "--median-filter-and-densify-iterations", "3"])
    assert (a.pyramid_level_for_depth, a.pyramid_level_for_color, a.median_filter_and_densify_iterations) == (1, 2, 3)


def test_levels_that_do_not_divide_the_dataset_size_are_refused():
    run_tum.check_level_fits(640, 480, 3)
    run_tum.check_level_fits(642, 481, 0)
    for width, height, level in ((642, 480, 2), (640, 481, 1), (640, 480, 4), (640, 480, -1)):
        with pytest.raises(ValueError):
            run_tum.check_level_fits(width, height, level)
