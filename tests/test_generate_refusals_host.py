"""Host: generate_indices.generate() on every combination of generate_flow_cases.REFUSAL_GRID (6 912 calls with paths that do not
exist) gives the outcome recorded in tests/golden/f13_generate_refusals.json by tools/record_generate_flows.py, before the refusals
became one ordered list: the same ValueError text where several refusals apply, FileNotFoundError where none does, and no file."""
import itertools
import json
import os

import generate_flow_cases as gfc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_every_combination_is_refused_as_recorded(tmp_path):
    from lcrec_amd import generate_indices as gen
    with open(os.path.join(GOLD, "f13_generate_refusals.json")) as fh:
        recorded = json.load(fh)
    assert recorded["grid"] == [[name, list(values)] for name, values in gfc.REFUSAL_GRID]
    outcomes, which = gfc.refusal_outcomes(gen, tmp_path)              # (asserts itself that no output file appeared)
    want = [recorded["outcomes"][ord(c) - ord("a")] for c in recorded["which"]]
    got = [outcomes[w] for w in which]
    assert len(got) == len(want) == 6912
    names = [name for name, _ in gfc.REFUSAL_GRID]
    for combo, g, w in zip(itertools.product(*(values for _, values in gfc.REFUSAL_GRID)), got, want):
        assert g == w, f"{dict(zip(names, combo))}: not the recorded outcome ({recorded['commit'][:12]})"
    assert os.listdir(tmp_path) == []
    # what the fixture is there to pin: `finish` is only looked at without --extend, which ignores it
    suffix_refusal = next(o for o in recorded["outcomes"] if o.startswith("finish='suffix'"))
    assert want.count(suffix_refusal) == 14 and want.count("FileNotFoundError") == 100 and len(recorded["outcomes"]) == 20
