"""No measurement switch without a test: every name cp_ctx_set_option accepts (core.h knob_names()) is forced by a row of a FORMS
table of the launch-form matrices, or names the test that covers it below, and has its row in INTEGRATION.md section 5b. CPU only:
importing the GPU modules must not touch a GPU."""
import os
import re

import test_gpu_air_forms
import test_gpu_merkle_forms
import test_gpu_ntt_forms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = (test_gpu_merkle_forms, test_gpu_ntt_forms, test_gpu_air_forms)

# switches the form matrices do not force, and the test module that does
EXCLUDED = {
    "QUOT_ALL_MAX": "test_gpu_gate_set.py",
    "QUOT_FLIP": "test_gpu_gate_set.py",
    "QUOT_GROUP": "test_gpu_gate_set.py",
    "QUOT_TILE": "test_gpu_gate_set.py",
    "DEVICE_TRANSCRIPT": "test_gpu_fri_generic.py",
    "COOP_FRI_MAX": "test_gpu_fri_generic.py",
}


def knob_names():
    src = open(os.path.join(ROOT, "city-rollup_amd", "csrc", "core.h")).read()
    body = re.search(r"knob_names\(\)\s*\{.*?names\[\]\s*=\s*\{(.*?)\};", src, re.S)
    assert body, "knob_names() not found in core.h"
    names = re.findall(r'"([A-Z0-9_]+)"', body.group(1))
    assert names and "nullptr" in body.group(1)
    return names


def test_knob_names_parse():
    names = knob_names()
    assert len(names) == len(set(names)) >= 15
    assert {"MERKLE_FUSE", "NTT_STAGED_STORE", "AIR_LDS_SLOTS"} <= set(names)


def test_every_switch_is_forced_by_a_form_matrix_or_excluded_by_name():
    names = set(knob_names())
    forms = {}
    for m in MODULES:
        for k, v in m.FORMS.items():
            assert v, "%s.FORMS[%s] names no case" % (m.__name__, k)
            forms.setdefault(k, []).append(m)
    assert not set(forms) & set(EXCLUDED), "a switch is both forced and excluded"
    assert set(forms) <= names, "FORMS names switches the library does not have: %s" % sorted(set(forms) - names)
    missing = names - set(forms) - set(EXCLUDED)
    assert not missing, "switches no form matrix forces: %s" % sorted(missing)
    assert set(EXCLUDED) <= names
    for k, mod in EXCLUDED.items():
        src = open(os.path.join(ROOT, "tests", mod)).read()
        assert k in src, "%s does not mention %s" % (mod, k)


def test_form_tables_name_existing_cases():
    rows = test_gpu_merkle_forms.ROWS
    for k, v in test_gpu_merkle_forms.FORMS.items():
        assert all(r in rows and k in rows[r][0] for r in v), k
    for m in (test_gpu_ntt_forms, test_gpu_air_forms):
        for k, v in m.FORMS.items():
            for name in v:
                fn = getattr(m, name, None)
                assert callable(fn) and name.startswith("test_"), (m.__name__, k, name)


def test_every_switch_has_a_row_in_integration_md():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## 5b."):]
    sec = sec[:sec.index("\n## ", 4)]
    rows = [line for line in sec.splitlines() if line.startswith("| `")]
    for name in knob_names():
        assert any("`CITYPROVER_%s`" % name in line.split("|")[1] for line in rows), name
