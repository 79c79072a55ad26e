"""The one chunk loop of ``GPPlan`` (``predict``, ``predict_terms``, ``predict_slopes``, ``predict_sensitivity``): the columns
``lo:hi`` of a chunked call equal, bit for bit, the same method called whole on ``Xs[..., lo:hi, :]`` alone -- the library's own
answer on identical inputs, so nothing is claimed about whole against chunked -- and a result that was not asked for stays None.

loadest d = 3 in float64, n = 129 (N = 256: pad rows exist), m = 257 with ``chunk=128``: three chunks, the last of one point;
one plan, and a ragged batch of two (129 and 70 rows)."""
import pytest
import torch

from tests.test_gpu_stages import make_case

pytestmark = pytest.mark.gpu

MODEL, D, M_POINTS, CHUNK = "loadest", 3, 257, 128
RANGES = [(0, 128), (128, 256), (256, 257)]


@pytest.fixture(scope="module", params=[(129,), (129, 70)], ids=["one-plan", "ragged-batch"])
def held(request, gpu_device):
    """-> (plan with a held factorisation, theta, Xs, diag, rhs) on the device; built once per configuration."""
    from discontinuum_amd import _lib
    from discontinuum_amd.backend import GPPlan

    dev, sizes = gpu_device, request.param
    B, n = len(sizes), max(sizes)
    lead = () if B == 1 else (B,)
    X, r, noise = torch.full((B, n, D), 0.3, dtype=torch.float64), torch.zeros(B, n, dtype=torch.float64), torch.ones(B, n, dtype=torch.float64)
    thetas = []
    for b, nb in enumerate(sizes):
        X[b, :nb], r[b, :nb], noise[b, :nb], th = make_case(MODEL, D, nb, seed=60 + b, perturb=0.2)
        thetas.append(th)
    theta = torch.stack(thetas).reshape(lead + (-1,))
    Xs = torch.stack([make_case(MODEL, D, M_POINTS, seed=70 + b)[0] for b in range(B)]).reshape(lead + (M_POINTS, D)).to(dev)
    g = torch.Generator().manual_seed(3)
    diag, rhs = (torch.randn(lead + (1, n), generator=g, dtype=torch.float64).to(dev) for _ in range(2))
    plan = GPPlan(MODEL, n, D, dtype=torch.float64, device=dev, batch=B)
    if B > 1:
        plan.set_site_sizes(sizes)
    plan.set_inputs(X.reshape(lead + (n, D)).to(dev).contiguous())
    out = plan.factorize(theta, r.reshape(lead + (n,)).to(dev).contiguous(), noise.reshape(lead + (n,)).to(dev).contiguous())
    assert bool((out[..., _lib.OUT_INFO] == 0).all())
    return plan, theta, Xs, diag, rhs


def _calls(plan, theta, diag, rhs):
    """name -> (call(Xs, chunk), which results are None)."""
    cols = list(range(D))
    return {
        "predict": (lambda xs, chunk: plan.predict(theta, xs, chunk=chunk), ()),
        "predict_terms": (lambda xs, chunk: plan.predict_terms(theta, xs, chunk=chunk), ()),
        "predict_terms_mean": (lambda xs, chunk: plan.predict_terms(theta, xs, chunk=chunk, return_cov=False), (1,)),
        "predict_slopes": (lambda xs, chunk: plan.predict_slopes(theta, xs, cols, chunk=chunk), ()),
        "predict_slopes_mean": (lambda xs, chunk: plan.predict_slopes(theta, xs, cols, chunk=chunk, return_cov=False), (1,)),
        "predict_sensitivity": (lambda xs, chunk: plan.predict_sensitivity(theta, xs, diag=diag, rhs=rhs, chunk=chunk), ()),
        "predict_sensitivity_mean": (lambda xs, chunk: plan.predict_sensitivity(theta, xs, diag=diag, rhs=rhs, chunk=chunk, return_var=False), (1,)),
    }


@pytest.mark.parametrize("name", ["predict", "predict_terms", "predict_terms_mean", "predict_slopes", "predict_slopes_mean",
                                  "predict_sensitivity", "predict_sensitivity_mean"])
def test_chunk_columns_are_the_library_answer_for_that_range(name, held):
    plan, theta, Xs, diag, rhs = held
    call, nones = _calls(plan, theta, diag, rhs)[name]
    chunked = call(Xs, CHUNK)
    assert len(chunked) == 2 and all((t is None) == (i in nones) for i, t in enumerate(chunked))
    for t in chunked:
        assert t is None or (t.shape[-1] == M_POINTS and t.is_contiguous())
    for lo, hi in RANGES:
        alone = call(Xs[..., lo:hi, :], None)  # one chunk: written in place, nothing staged
        for i, (a, c) in enumerate(zip(alone, chunked)):
            assert (a is None) == (i in nones)
            if a is not None:
                assert a.shape[-1] == hi - lo and torch.equal(c[..., lo:hi], a), (name, i, lo, hi)
