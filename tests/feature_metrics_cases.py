"""Seeded feature sets for the feature-metric tests: ReLU features on a 6-dimensional latent, so that the k-NN manifolds of a "real" and a
"fake" set overlap partly - precision, recall, density and coverage all lie strictly between their trivial values in most cases - and every
comparison of a distance with a radius is far (>= 1e-5 of the largest d2) from its threshold, where float64 error is about 1e-12."""
import functools

import numpy as np

from tests import feature_metrics_restatement as fm

LATENT = 6
DIMS = (2048, 70)
SETS = ((65, 63, 0.0, 1.0), (65, 63, 0.7, 1.0), (130, 33, 0.0, 0.5), (33, 130, 1.5, 1.0), (257, 64, 0.4, 0.8))       # N, M, shift, scale of the fake set
CASES = tuple((n, m, shift, scale, d) for d in DIMS for (n, m, shift, scale) in SETS)
KS = (1, 3, 5)


def case_id(c):
    return f"N{c[0]}-M{c[1]}-shift{c[2]}-scale{c[3]}-D{c[4]}"


@functools.lru_cache(maxsize=None)
def _basis(dim):
    g = np.random.default_rng(1234)
    a = g.standard_normal((LATENT, dim)) / np.sqrt(LATENT)
    b = 0.3 * g.standard_normal(dim)
    return a, b


def feats(seed, n, shift, scale, dim):
    a, b = _basis(dim)
    z = scale * np.random.default_rng(seed).standard_normal((n, LATENT)) + shift
    return np.maximum(z @ a + b, 0.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sets(case):
    n, m, shift, scale, dim = case
    real, fake = feats(1, n, 0.0, 1.0, dim), feats(2, m, shift, scale, dim)
    real.setflags(write=False)
    fake.setflags(write=False)
    return real, fake


@functools.lru_cache(maxsize=None)
def reference(case, k):
    return fm.prc(*sets(case), k)


def signed(n, dim, seed):
    """Signed features whose magnitudes span 1e-3 .. 1e3: sum |a b| is far above |g|, the regime the bound on g is written for."""
    g = np.random.default_rng(seed)
    return (g.choice([-1.0, 1.0], (n, dim)) * 10.0 ** g.uniform(-3.0, 3.0, (n, dim))).astype(np.float32)


def random_features(n, dim, seed):
    g = np.random.default_rng(seed)
    return np.maximum(g.standard_normal((n, dim)) + 0.3, 0.0).astype(np.float32)
