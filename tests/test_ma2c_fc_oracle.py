"""MA2C with the feed-forward fingerprint policy (the reference's FPFcACPolicy, agents/policies.py:259-282) on the CPU:
the float64 restatement oracle/nets_oracle.py replays the two episodes recorded from the reference's own learner code
(tools/make_golden_fpfc.py -> tests/golden/refnet_ma2c_fc_{large,real}.npz), exactly as tests/test_refnet_oracle.py
does for the other A2C fixtures: the initial weights under the recorded np.random seed, every pi / v, the float32
returns and advantages, the raw gradient of every variable, the per-agent norms, and the variables and RMSProp slots
after each update.  Net: fcw(wave -> 128) | fcf(fingerprint -> 64) | fct(wait -> 32), fc(H -> 64), heads; H = 224 on
large_grid, 192 on Monaco (no wait inputs)."""
import numpy as np
import pytest

from oracle import refnet
from tests.test_refnet_oracle import test_oracle_replays_reference_learner as _replay
from tests.test_refnet_oracle import test_reference_weights_under_seed as _weights

FIXTURES = ['refnet_ma2c_fc_large', 'refnet_ma2c_fc_real']


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_is_the_fingerprint_fc_net(name):
    """The recording holds FPFcACPolicy variables (fcw | fcf | [fct] | fc, no LSTM) of widths 128 / 64 / 32 / 64."""
    fx = refnet.load_fixture(name)
    assert str(fx['agent']) == 'ma2c' and str(fx['policy']) == 'fc'
    want = refnet.unpack_digests(fx['w0/names'], fx['w0/rows'])
    keys = {k.split('/')[1] for k in want}
    has_wait = max(fx['n_w_ls'].tolist()) > 0
    assert keys == {'fcw_w', 'fcw_b', 'fcf_w', 'fcf_b', 'fc_w', 'fc_b', 'out_w', 'out_b'} | ({'fct_w', 'fct_b'} if has_wait else set())
    n_wave, n_w, n_f, n_a, n_fc = refnet.fixture_dims(fx)
    assert n_fc == (128, 64, 32 if has_wait else 0) and min(n_f) > 0
    towers = refnet.initial_towers(fx)
    assert towers[0]['fc_w'].shape == (sum(n_fc), 64) and towers[0]['fcf_w'].shape == (n_f[0], 64)
    assert int(fx['n_backward']) == (1 if str(fx['scenario']) == 'large_grid' else 3)


@pytest.mark.parametrize('name', FIXTURES)
def test_reference_weights_under_seed(name):
    _weights(name)


@pytest.mark.parametrize('name', FIXTURES)
def test_oracle_replays_reference_learner(name):
    _replay(name)


def test_fingerprint_inputs_reach_the_fcf_block():
    """The recorded pi depends on the fingerprint inputs through fcf: zeroing them in the oracle changes the policy."""
    from oracle.nets_oracle import OracleA2C
    fx = refnet.load_fixture('refnet_ma2c_fc_large')
    n_wave, n_w, n_f, n_a, n_fc = refnet.fixture_dims(fx)
    o = OracleA2C(refnet.initial_towers(fx), n_wave, n_w, n_f, n_a, 1)
    o.reset()
    obs = fx['fw_obs'][5][None].astype(np.float64)
    pis, _ = o.forward(obs, False, 'pv')
    cut = obs.copy()
    for a in range(len(n_a)):
        cut[0, a, n_wave[a] + n_w[a]:n_wave[a] + n_w[a] + n_f[a]] = 0.0
    pis2, _ = o.forward(cut, False, 'pv')
    assert max(np.abs(pis[a][0] - fx['fw_pi'][5, a, :n_a[a]]).max() for a in range(len(n_a))) < 1e-12
    assert max(np.abs(pis[a][0] - pis2[a][0]).max() for a in range(len(n_a))) > 1e-6
