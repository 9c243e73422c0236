"""The caps of the assignment calls (csrc/ctg_take.hip) past which a loop takes
a second turn or the count slots change, mirrored once for
tests/test_gpu_take.py; tests/test_take_host.py (test_cap_mirrors) pins each
against the plan function or the launch's own text."""
CHUNK = 4096                  # csrc/ctg_plan.h: TAKE_CHUNK, voxels a workgroup of k_take
MAX_TURN = 4096 * 256         # csrc/ctg_take.hip: launch_take_max, at most 4096 workgroups of 256 threads, an entry each a turn
SLOTS = 64                    # csrc/ctg_plan.h: take_count_slots, count slots a segment ...
SLOT_SEGMENTS = 4096          # ... up to this many segments; one slot beyond


def count_slots(n_seg):
    return SLOTS if n_seg <= SLOT_SEGMENTS else 1


def max_turns(n):
    """Turns of k_take_max's grid-stride loop over a dense table of n entries."""
    return -(-n // MAX_TURN)
