"""The classification of the workspace slots is written down twice — ws_table in csrc/selftest.hip (what cn_selftest_ws_fill acts on) and the
table of DESIGN.md section 3.1 — and the enum of csrc/common.hpp is the third list of the slots: the three agree.  No GPU needed."""
import os
import re

import selftest_bind as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def design_rows():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 3.1 The workspaces"):text.index("## 4. Kernels")]
    rows = re.findall(r"^\| `(WS_[A-Z0-9_]+)` \| ([^|]+) \| (scratch|vouched|polled) \| ([^|]*) \|$", sec, flags=re.M)
    return [(n, stage.strip(), cls, why.strip()) for n, stage, cls, why in rows]


def enum_names(first, stop):
    src = open(os.path.join(ROOT, "cornetto_amd", "csrc", "common.hpp")).read()
    body = src[src.index(first):src.index(stop)]
    return re.findall(r"\b((?:WS|PIN)_[A-Z0-9_]+)\b", body)


def test_the_hook_names_every_slot_of_the_enums_in_order():
    assert st.ws_names() == enum_names("WS_TF_LUT,", "WS_COUNT")
    assert st.pin_names() == enum_names("PIN_A,", "PIN_COUNT")


def test_design_table_equals_the_hooks_table():
    rows = design_rows()
    classes = st.ws_classes()
    assert [r[0] for r in rows] == list(classes)                       # one row per slot, in the order of the enum
    for name, stage, cls, why in rows:
        hook_cls, voucher = classes[name]
        assert cls == hook_cls and stage, name
        if cls == "scratch":
            assert why == "" and voucher == ""
        else:                                                          # every other row names its voucher or says "polled", as the hook does
            assert voucher and all("`%s`" % f in why for f in voucher.split(", ")), name
            assert (cls == "polled") == why.startswith("polled"), name
    assert {n for n, (c, _) in classes.items() if c == "polled"} == {"WS_SCAN", "WS_STITCH"}
    assert {n for n, (c, _) in classes.items() if c == "vouched"} == {"WS_TF_LUT", "WS_TF_BITMAP"}
