"""No device needed: the leaf-net entries answer every descriptor of the recorded grid as they did when
tests/golden/leafnet_descriptor_table.json was written (make_leafnet_descriptor_table.py, against the commit before the host side
was split into family units): azmi_net_blob_bytes, azmi_net_blob_bytes2, and the code and full text of azmi_net_create /
azmi_net_create2.  A descriptor the library accepts was recorded without a device (AZMI_ERR_NO_DEVICE, "no HIP device"); with
one it yields a net, which is destroyed.  Nothing else may differ.  No kernel runs.
"""
import json

import pytest

import make_leafnet_descriptor_table as mk


@pytest.fixture(scope="module")
def lib():
    from alphazero import _capi
    return mk.load(_capi.LIB_PATH)


@pytest.fixture(scope="module")
def table():
    with open(mk.TABLE) as f:
        return json.load(f)


def test_the_grid_is_the_recorded_one(table):
    assert [name for name, _, _ in mk.grid()] == list(table["rows"])


def test_every_size_code_and_text_is_the_recorded_one(lib, table):
    texts, wrong = table["texts"], []
    for name, words, delta in mk.grid():
        b1, b2, rc1, t1, rc2, t2 = table["rows"][name]
        got = mk.answers(lib, words, delta)
        want = [b1, b2, rc1, texts[t1], rc2, texts[t2]]
        for k in (2, 4):      # an accepted descriptor: recorded without a device, a net with one
            if mk.accepted(want[k], want[k + 1]) and got[k] == mk.AZMI_OK:
                got[k], got[k + 1] = want[k], want[k + 1]
        if got != want:
            wrong.append((name, got, want))
    assert not wrong, "%d rows differ, the first: %r" % (len(wrong), wrong[0])


def test_the_table_holds_an_accepted_row_per_family_and_a_refusal_per_text(table):
    import re
    texts = table["texts"]
    for pattern in mk.REFUSALS:
        assert any(re.fullmatch(pattern, t) for t in texts), pattern
    for name in mk.BASES:
        r = table["rows"][name + "/base"]
        assert r[1] > 0 and mk.accepted(r[4], texts[r[5]]), name
