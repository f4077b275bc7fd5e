"""The primitive edge fuzz (tests/prim_fuzz.py) on the HIP library against the
oracle, bit for bit in every returned item -- f64 buffer, u8 buffer, get_color
probes, the booleans of set_pixel / apply_pixel / restore_state, every texture
made by resample / as_texure -- on the four submission paths: immediate
(k_prim and the pixel kernels), recorded (k_cmd_list), packed
(ExecuteCommands) and packed while recording.

tests/test_prim_fuzz.py checks on the CPU that the cases reach the branches
they are built for; the module docstring of prim_fuzz.py lists what is left out.
On a mismatch the case is re-run in growing prefixes on both sides and the
failure names the first operation after which the buffers differ."""
import functools

import pytest

import prim_fuzz as P
import scenes

pytestmark = pytest.mark.gpu

PATHS = {
    "immediate": lambda: scenes.GpuFactory(),
    "recorded": lambda: scenes.GpuRecordingFactory(),
    "packed": lambda: scenes.GpuPackedFactory(False),
    "packed-recording": lambda: scenes.GpuPackedFactory(True),
}


@functools.lru_cache(maxsize=None)
def _case(family, seed):
    return P.FAMILIES[family][0](seed)


@functools.lru_cache(maxsize=None)
def _want(family, seed):
    """The oracle's outputs, computed once per case and shared by the four paths."""
    return P.run(_case(family, seed), scenes.OracleFactory())


def _first_differing_op(case, fac, ora):
    for n in range(1, len(case["ops"]) + 1):
        if P.mismatches(P.run(case, fac, upto=n), P.run(case, ora, upto=n)):
            return P.describe(case, n - 1, ora)
    return "no prefix differs (only the whole case does)"


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("family,seed", P.case_ids(), ids=lambda v: str(v))
def test_case_matches_oracle(gpu, oracle, family, seed, path):
    case = _case(family, seed)
    fac = PATHS[path]()
    got = P.run(case, fac)
    want = _want(family, seed)
    bad = P.mismatches(got, want)
    if bad:
        pytest.fail(f"{case['name']} on {path}: {bad}; {_first_differing_op(case, fac, oracle)}")
    if path in ("immediate", "recorded"):
        assert None not in got["bools"]                    # these paths return every boolean
    # a recording context still holds exactly the commands each list_len names (none was run early,
    # none was dropped, recording did not stop); a context that is not recording holds none
    named = [op[1] for op in case["ops"] if op[0] == "list_len"]
    recording = path in ("recorded", "packed-recording")
    assert got["list_len"] == (named if recording else [None] * len(named)), (case["name"], path)
