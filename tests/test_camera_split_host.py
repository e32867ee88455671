"""CPU (-m "not gpu"): the host arithmetic that divides a launch's persistent workgroups between the two cameras' jobs of one encoder stage
(common.h::camera_split through hulc_k_camera_split).  No device needed."""
import ctypes as C


def _split(lib, grid, ws, wg):
    a, b = C.c_int32(-1), C.c_int32(-1)
    assert lib.hulc_k_camera_split(grid, float(ws), float(wg), C.byref(a), C.byref(b)) == 0
    return a.value, b.value


GRIDS = (2, 3, 5, 16, 255, 256, 512, 1024)
# items x rounds per item as the launchers count them: a handful of frames up to the 2048-frame step, 1 .. 4 rounds
WORKS = sorted({i * r for i in (1, 2, 3, 7, 64, 293, 512, 2048, 6144) for r in (1, 2, 3, 4)})


def test_both_jobs_get_a_workgroup_and_the_counts_sum_to_the_grid():
    from hulc_amd import lib as L
    lib = L.load()
    for grid in GRIDS:
        for ws in WORKS:
            for wg in WORKS:
                a, b = _split(lib, grid, ws, wg)
                assert a >= 1 and b >= 1, (grid, ws, wg, a, b)
                assert a + b == grid, (grid, ws, wg, a, b)


def test_gripper_share_is_the_rounded_work_share_and_never_shrinks_as_its_work_grows():
    from hulc_amd import lib as L
    lib = L.load()
    for grid in GRIDS:
        for ws in WORKS:
            prev = 0
            for wg in WORKS:                      # ascending
                a, b = _split(lib, grid, ws, wg)
                assert b >= prev, (grid, ws, wg, b, prev)
                prev = b
                want = min(max(int(grid * (wg / (ws + wg)) + 0.5), 1), grid - 1)
                assert b == want, (grid, ws, wg, b, want)


def test_one_job_takes_the_whole_grid():
    from hulc_amd import lib as L
    lib = L.load()
    for grid in (1,) + GRIDS:
        for ws in WORKS:
            assert _split(lib, grid, ws, 0) == (grid, 0)


def test_the_step_shapes_give_the_gripper_camera_about_its_pixel_share():
    """conv3 forward of the 2048-frame step in the cost model's units, the launcher's FIRST division: 2048 static items of 2 wave passes against 293 gripper
    items (7 frames stacked, the stack a whole grid would get) of 3 passes, each + 0.35 of fixed cost per item: 17 % of the work, 43 of 256 workgroups.  (The
    launcher then re-plans the gripper stack for those 43 workgroups and divides once more with the new item count; the function is the same.)"""
    from hulc_amd import lib as L
    lib = L.load()
    assert _split(lib, 256, 2048 * 2.35, 293 * 3.35) == (213, 43)
