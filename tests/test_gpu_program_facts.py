"""What hnb_program_kernel_info says statically about one program of every kind the creation-time proofs (csrc/hnb_program.h) tell
apart - plain streaming, generic update, one AGE_TICK, a ribbon trail whose front is static and one whose is not, a kill modifier, an event
parent and its child, cohorts on, cohorts off by HNB_AGE_COHORT_AUTO - is what the library said before the proofs moved into the header
(tests/golden/program_kernel_info.json, written by tests/golden/make_program_goldens.py kernel-info): one instance each, two frames."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_program_goldens as gold  # noqa: E402


@pytest.mark.gpu
def test_kernel_info_of_every_kind_of_program_is_the_recorded_one():
    want = json.load(open(gold.KERNEL_INFO_PATH))
    got = gold.kernel_info_record()
    assert set(got) == set(want) == set(gold.kernel_info_cases())
    for name in want:
        assert got[name] == want[name], name
    # the record tells the kinds apart by the markers the proofs decide
    text = {name: "\n".join(lines) for name, lines in want.items()}
    not_eligible = lambda name, line: any(l.startswith(line) and l.endswith("(not eligible)") for l in want[name])
    assert not not_eligible("firework_streaming_cohort_off_by_auto", "lists skipped") and not_eligible("kill_modifier", "lists skipped")
    assert not_eligible("generic_update", "lists skipped") and not_eligible("event_parent", "lists skipped") and not_eligible("event_child", "lists skipped")
    assert "death horizons in use" in text["firework_streaming_cohort_off_by_auto"] and "death horizons in use" not in text["kill_modifier"]
    assert "death horizons in use" not in text["one_age_tick_ribbon_front_static"] and "death horizons in use" not in text["generic_update"]
    assert not not_eligible("one_age_tick_ribbon_front_static", "ribbon sorts by rotation") and not_eligible("ribbon_not_front_static", "ribbon sorts by rotation")
    assert "age cohorts: off (HNB_AGE_COHORT_AUTO" in text["cohort_off_by_auto_4096"] and "age cohorts: # of # chunks" in text["cohort_on_render_ignores_age"]
    assert "the update keeps the plane current" in text["cohort_on_auto_65536"]
    assert want["one_age_tick_ribbon_front_static"][0] == "init=jit update=aot-stream:ProgAge" and want["generic_update"][0] == "init=jit update=jit-generic"
