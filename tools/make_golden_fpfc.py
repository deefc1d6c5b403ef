#!/usr/bin/env python
"""Generate the MA2C + FC-policy reference fixtures (build container only; needs the reference checkout).

The reference defines the fingerprint variant of its feed-forward policy, FPFcACPolicy (agents/policies.py:259-282),
but agents/models.py never builds it and its _build_net reads a free name `ob` where `self.obs` is meant.
This runs oracle.refnet.run_reference_a2c(agent='ma2c', policy='fc') with three patches made at run time, after the
reference modules are imported over oracle/fake_tf.py -- no reference source is copied or edited:
  * MA2C._init_policy builds FPFcACPolicy with the config's num_fw / num_ft / num_fp / num_lstm;
  * MA2C.reset does nothing (the FC policies are stateless and have no _reset);
  * FPFcACPolicy._build_net binds the module-level name `ob` to the instance's `self.obs`, then runs unchanged.
Net: fcw(wave -> 128) | fcf(fingerprint -> 64) | fct(wait -> 32), concatenated in that order, fc(H -> 64), heads.

    python tools/make_golden_fpfc.py       # writes tests/golden/refnet_ma2c_fc_{large,real}.npz
      refnet_ma2c_fc_large .. config_ma2c_large.ini, 600 s = 120 steps, one update (H = 224)
      refnet_ma2c_fc_real ... config_ma2c_real.ini, 600 s = 3 x 40 steps (28 agents, no wait inputs: H = 192)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'tests', 'golden')

from oracle import refnet                                      # noqa: E402

FIXTURES = (('refnet_ma2c_fc_large', dict(scenario='large_grid', agent='ma2c', seed_w=107, episode_sec=600, policy='fc')),
            ('refnet_ma2c_fc_real', dict(scenario='real_net', agent='ma2c', seed_w=108, episode_sec=600, policy='fc')))


def _patch_reference():
    """Applied right after refnet._install() has (re)imported the reference's agents package."""
    import agents.models as ref_models
    import agents.policies as ref_policies
    base = ref_policies.FPFcACPolicy

    class FPFcBound(base):
        def _build_net(self, out_type):
            ref_policies.ob = self.obs                  # the free name of the reference method
            try:
                return base._build_net(self, out_type)
            finally:
                del ref_policies.ob

    def _init_policy(self, n_s, n_a, n_w, n_f, model_config, agent_name=None):
        return FPFcBound(n_s, n_a, n_w, n_f, self.n_step, n_fc_wave=model_config.getint('num_fw'),
                         n_fc_wait=model_config.getint('num_ft'), n_fc_fp=model_config.getint('num_fp'),
                         n_lstm=model_config.getint('num_lstm'), name=agent_name)

    def reset(self):
        pass

    ref_models.MA2C._init_policy = _init_policy
    ref_models.MA2C.reset = reset


def main():
    orig = refnet._install

    def install():
        out = orig()
        _patch_reference()
        return out
    refnet._install = install
    try:
        for name, kw in FIXTURES:
            fx = refnet.run_reference_a2c(**kw)
            assert all(k.split('/')[-1] != 'lstm_wx' for k in refnet.unpack_digests(fx['w0/names'], fx['w0/rows'])), name
            path = os.path.join(OUT, name + '.npz')
            np.savez_compressed(path, **fx)
            print(path, os.path.getsize(path))
    finally:
        refnet._install = orig


if __name__ == '__main__':
    main()
