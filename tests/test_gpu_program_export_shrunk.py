"""The three program exports that keep a scratch per program - hnb_program_export_sorted (instance scope), hnb_program_export_filtered and
hnb_program_export_sorted with an HnbExportSortFiltered - over a program that LOST an instance after those scratches were allocated: the sections
stay where the allocation for three instances put them while the grids are those of the two instances left, and the first instance's place in the
tables is taken by the last. Then the program gains instances and the scratches are regrown. Every call is compared as the forms' own tests
compare it: bit for bit with the per-effect calls and the host's restatement."""
import pytest

import test_gpu_program_export_filtered as pef
import test_gpu_program_export_sorted as pes
from test_gpu_export_filtered import HALF
from test_gpu_program_export_filtered import BASES, fx_slot_base, make_based
from test_gpu_program_export_filtered_sorted import DEPTH, check
from test_gpu_program_export_sorted import POS_AGE_ID, step

pytestmark = pytest.mark.gpu


def check_three_forms(ctx, prog, fxs, what):
    """fxs in table order. One depth key, one plane that keeps part of each instance, records of 20 bytes."""
    pes.check(ctx, prog, fxs, what, "instance", POS_AGE_ID, 20, [fx_slot_base(fx) for fx in fxs], **DEPTH)
    pef.check(ctx, prog, fxs, what, HALF)
    check(ctx, prog, fxs, what, HALF, DEPTH)


@pytest.mark.parametrize("cap", [4096, 4097])                            # one workgroup per instance | two tiles: the sorts zero their state words and group sums
def test_a_program_that_lost_its_first_instance_and_then_gains_two(cap):
    ctx, prog, fxs = make_based(cap, 3)
    step(ctx, fxs, 0, [cap, cap - 1, cap // 2])
    check_three_forms(ctx, prog, fxs, "three instances")                 # the scratches are allocated for three
    fxs[0].destroy()                                                     # the last instance is moved into its place
    fxs = [fxs[2], fxs[1]]
    assert [fx.index() for fx in fxs] == [0, 1] and [fx_slot_base(fx) for fx in fxs] == [BASES[2], BASES[1]]
    step(ctx, fxs, 1, [0, 0], dt=0.3)
    ctx.synchronize()
    assert all(0 < fx.alive_count() < cap for fx in fxs)
    check_three_forms(ctx, prog, fxs, "two instances in the scratches of three")
    for base in BASES[3:5]:                                              # four instances: the scratches are regrown
        fx = prog.create_effect(slot_base=base)
        fx.slot_base_given = base
        fxs.append(fx)
    step(ctx, fxs, 2, [0, 0, cap - 1, cap // 3])
    check_three_forms(ctx, prog, fxs, "four instances")
    ctx.close()
