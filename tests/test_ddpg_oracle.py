"""The CPU restatement of the reference DDPGTrainer step (tests/ddpg_oracle.py)
against the reference's own runs (tests/golden/ddpg_*.npz,
make_golden_ddpg.py), and proof that the fixtures pin the torch-1.4 update
order."""
import pytest
import torch

import ddpg_oracle as do
import parity

FIXTURES = ["ddpg_small", "ddpg_fixed_std", "ddpg_tpn", "ddpg_stress", "ddpg_humanoid"]


@pytest.mark.parametrize("name", FIXTURES)
def test_ddpg_oracle_matches_reference_golden(name):
    """The float32 oracle meets parity.gate on every golden key, every step,
    with no row left out."""
    meta, g = parity.load(name)
    errs = do.oracle_errors(meta, g, do.make_oracle(meta, g))
    assert set(errs) == do.golden_keys(g)
    noise = do.noise_of(meta, g)
    bad = {k: (v, noise[k]) for k, v in errs.items() if v > parity.gate(k, noise[k])}
    print(name, "worst", sorted(errs.items(), key=lambda kv: -kv[1])[:3])
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0])[:10]


@pytest.mark.parametrize("name", FIXTURES)
def test_ddpg_stats_key_order(name):
    meta, g = parity.load(name)
    keys = [k[len("s0/stat/"):] for k in g if k.startswith("s0/stat/")]
    assert keys == do.STAT_KEYS


def test_fixtures_pin_the_update_order():
    """Sending the policy gradient through the PRE-step critic misses the gate
    on every policy gradient tensor of ddpg_fixed_std step 0 by >= 100x."""
    meta, g = parity.load("ddpg_fixed_std")
    meta = dict(meta, steps=1)
    errs = do.oracle_errors(meta, g, do.make_oracle(meta, g, quirk=False))
    noise = do.noise_of(meta, g)
    for pn in do.POLICY_KEYS:
        key = f"s0/grad/policy/{pn}"
        print(key, errs[key], parity.gate(key, noise[key]))
        assert errs[key] >= 100.0 * parity.gate(key, noise[key]), (key, errs[key])
    # and with the ordering modelled the same tensors pass
    ok = do.oracle_errors(meta, g, do.make_oracle(meta, g))
    for pn in do.POLICY_KEYS:
        key = f"s0/grad/policy/{pn}"
        assert ok[key] <= parity.gate(key, noise[key]), (key, ok[key])
