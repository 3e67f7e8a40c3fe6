"""The unit decoder's first layer on the distinct rows (ss_batch_t2u_units, ss_batch_t2u_units_pad; csrc/batch.hip).

The unit decoder's input is ctc_upsample = 25 copies of every text-decoder state's row, so with pack-invariant arithmetic on the
LayerNorm and the QKV linear of its first layer run over the distinct rows and a copy kernel writes each result row 25 times.  That
must not move a bit: the switch ss_debug_unit_l0_distinct(0) puts both back on all upsampled rows, and the raw arg-max ids, the
collapsed units and the dense logits of the two forms are compared with torch.equal -- on a pack of 1, 2 and 7 states (25, 50 and
175 unit rows: one state is the smallest case, 7 states cross a 48-row tile), through the entry with trailing pads, and for the third
utterance alone against its rows in the pack.  With pack-invariant arithmetic off the old path must run whatever the switch says:
the launch census (ss_prof_shape_log) then counts the unit decoder's QKV rows.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

N_STATES = [1, 2, 7]
PADS = [0, 1, 2]


@pytest.fixture()
def switch(hip_model):
    lib = hip_model.lib

    def set_on(on):
        assert lib.ss_debug_unit_l0_distinct(int(on)) == 0
    yield set_on
    assert lib.ss_debug_unit_l0_distinct(-1) == 0


@pytest.fixture(scope="module")
def feats(hip_model):
    g = torch.Generator().manual_seed(2510)
    return torch.randn((len(N_STATES), max(N_STATES), hip_model.cfg.dec_dim), generator=g).cuda()


def _run(m, feats, n, pads=None):
    if pads is None:
        units, raw = m.batch_t2u_units(feats, n, return_raw=True)
    else:
        units, raw = m.batch_t2u_units_pad(feats, n, pads, return_raw=True)
    return units, raw, m.last_logits().clone()


@pytest.mark.parametrize("pads", [None, PADS], ids=["plain", "pad"])
def test_distinct_rows_give_the_same_bits(hip_model, switch, feats, pads):
    m = hip_model
    assert m.pack_invariant()
    switch(1)
    units1, raw1, log1 = _run(m, feats, N_STATES, pads)
    switch(0)
    units0, raw0, log0 = _run(m, feats, N_STATES, pads)
    assert log1.shape == (m.cfg.ctc_upsample * sum(N_STATES), m.cfg.unit_vocab)
    assert torch.isfinite(log0).all()
    assert torch.equal(torch.tensor(sum(raw1, [])), torch.tensor(sum(raw0, []))), "raw arg-max ids differ"
    assert units1 == units0, "collapsed units differ"
    assert torch.equal(log1, log0), "unit logits differ between the distinct-row and the all-row first layer"


@pytest.mark.parametrize("pads", [None, PADS], ids=["plain", "pad"])
def test_alone_equals_in_pack(hip_model, switch, feats, pads):
    """The third utterance alone (a pack of one) against its rows in the pack, both on the new path: bitwise."""
    m = hip_model
    switch(1)
    units, raw, log = _run(m, feats, N_STATES, pads)
    b = 2
    u1, r1, l1 = _run(m, feats[b:b + 1].contiguous(), N_STATES[b:], None if pads is None else pads[b:])
    o = m.cfg.ctc_upsample * sum(N_STATES[:b])
    assert torch.equal(l1, log[o:]), "logits of the utterance alone differ from its rows in the pack"
    assert r1[0] == raw[b] and u1[0] == units[b]


def _qkv_rows(lib, D):
    """Rows of the N = 3 D, K = D linears logged since ss_prof_shape_log(1): (launches, launches x mean rows summed over classes)."""
    n = lib.ss_prof_shape_dump(None, 0)
    buf = C.create_string_buffer(n)
    lib.ss_prof_shape_dump(buf, n)
    launches, rows = 0, 0.0
    for line in buf.value.decode().splitlines()[1:]:
        f = line.split()
        if int(f[1]) == 3 * D and int(f[2]) == 1 and int(f[3]) == D:
            launches += int(f[5])
            rows += int(f[5]) * float(f[6])
    return launches, rows


@pytest.mark.parametrize("invariant", [True, False], ids=["pack-invariant", "fastest-kernel"])
def test_launch_census(hip_model, switch, feats, invariant):
    """The QKV launches of one call: every T2U encoder layer over Nn rows, the unit decoder's layers over U = 25 Nn rows -- but its
    first layer over Nn rows on the new path, which only pack-invariant arithmetic may take."""
    m, cfg = hip_model, hip_model.cfg
    Nn, up = sum(N_STATES), hip_model.cfg.ctc_upsample
    switch(1)
    m.set_pack_invariant(invariant)
    try:
        m.lib.ss_prof_shape_log(1)
        _run(m, feats, N_STATES)
        launches, rows = _qkv_rows(m.lib, cfg.dec_dim)
    finally:
        m.lib.ss_prof_shape_log(0)
        m.set_pack_invariant(True)
    assert launches == cfg.t2u_layers + cfg.unit_layers
    first = Nn if invariant else up * Nn
    want = cfg.t2u_layers * Nn + first + (cfg.unit_layers - 1) * up * Nn
    assert abs(rows - want) <= launches, (rows, want)        # (the table prints mean rows per shape as whole numbers)


def test_switch_refuses_other_values(hip_model):
    assert hip_model.lib.ss_debug_unit_l0_distinct(2) == 2 and hip_model.lib.ss_debug_unit_l0_distinct(-2) == 2
