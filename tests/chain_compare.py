"""Comparison of a device chain with the CPU restatement's (oracle/sampler_oracle.py), shared by the sampler tests."""
import numpy as np


def compare_chains(chain, lps, ochain, olps):
    """Identical accept decisions -> identical positions; a decision can only differ when
    lnpdiff - log u is within rounding of 0, which does not happen on these seeds."""
    np.testing.assert_allclose(chain, ochain, rtol=1e-12, atol=1e-12)
    fin = np.isfinite(olps)
    assert np.array_equal(fin, np.isfinite(lps))
    np.testing.assert_allclose(lps[fin], olps[fin], rtol=1e-8)
