"""PREALPS_ECG_SOLVE_FIRST without a GPU: the switch is read as a solver reads it when it is reset, and the order
with the block solve first applies only to the one configuration it was made for; every other one keeps the order
of preAlps_ECGIterate."""
import os

import pytest

import prealps_amd as pa

# nprocs, ortho_alg, bs_red, enlFac, fuse, lazy_norm, lazy_stop, bj_gram, spmm_gram, graphs
HEADLINE = dict(nprocs=1, ortho_alg=pa.ORTHODIR, bs_red=pa.NO_BS_RED, enlFac=4, fuse=1, lazy_norm=1, lazy_stop=1,
                bj_gram=1, spmm_gram=1, graphs=0)
KEYS = list(HEADLINE)


def _rule(**kw):
    cfg = dict(HEADLINE, **kw)
    return pa.load().preAlps_hip_ecg_solve_first(*[int(cfg[k]) for k in KEYS])


@pytest.fixture
def switch(monkeypatch):
    def set_(v):
        if v is None:
            monkeypatch.delenv("PREALPS_ECG_SOLVE_FIRST", raising=False)
        else:
            monkeypatch.setenv("PREALPS_ECG_SOLVE_FIRST", v)
    return set_


def test_switch_is_read_and_defaults_on(switch):
    switch(None)
    assert _rule() == 1
    switch("1")
    assert _rule() == 1
    switch("0")
    assert _rule() == 0
    switch(None)
    assert _rule() == 1


@pytest.mark.parametrize("change", [
    dict(nprocs=2), dict(nprocs=8),                                   # several processes (and the shard rehearsal)
    dict(ortho_alg=pa.ORTHOMIN), dict(ortho_alg=pa.ORTHODIR_FUSED),    # Orthomin, fused Orthodir
    dict(bs_red=pa.ADAPT_BS),                                          # D-Odir / BF-Omin
    dict(enlFac=2), dict(enlFac=8), dict(enlFac=16),                   # t != 4
    dict(fuse=0), dict(lazy_norm=0), dict(lazy_stop=0),                # PREALPS_ECG_FUSE / LAZY_NORM / LAZY_STOP = 0
    dict(bj_gram=0), dict(spmm_gram=0),                                # no Gram block from the block solve / SpMM
    dict(graphs=1),                                                    # HIP graphs
], ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_every_other_configuration_keeps_todays_order(switch, change):
    switch(None)
    assert _rule(**change) == 0
    switch("1")
    assert _rule(**change) == 0
