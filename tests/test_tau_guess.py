"""The starting threshold of k_encode_prune's screening pass, on the host.

csrc/cwq_tau_guess.h predicts, from a tile's screening constants (alpha_j,
beta_j), the level q_m that on average m of the tile's N candidates' screened
sums Q = sum_j (alpha_j z_j + beta_j)^2 fall below: the Lugannani-Rice tail of
a weighted noncentral chi-square solved for P = m / N.
tests/native/tau_guess_check.cpp runs the header on the blocks below; it is
compiled and run once.  Checked here:

  * q_m against the same formula written out in float64 (bisection);
  * calibration by Monte Carlo with numpy normals, N = 2^bits rows per block;
  * "no guess" for the inputs the header must refuse.

The kernel needs none of this for its results (it verifies the guess at the
end of every tile and retries without it); a guess that is too high costs a
retry, one that is too low gains nothing, which is what is checked.
"""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from compression_without_quantization_amd.synthetic import make_blocks

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(8, 12, 400), (16, 12, 300), (64, 13, 200), (32, 16, 64)]   # (d, bits, nb)
# The header works in float32 and stops at |ln P - ln(m/N)| <= 2^-12, then
# takes one more Newton step on q; the largest relative difference from the
# float64 root measured over all blocks below (both steps) is 2.9e-6 (d = 8;
# 2.6e-6, 1.5e-6 and 1.1e-6 at d = 16, 64 and 32); the bound is four times that.
Q_RTOL = 1.2e-5


def _consts(d, bits, nb):
    """[nb, d, 5] float32: loc_s, scale_s, mu, sigma, best of a one-step call."""
    b = make_blocks(nb, d, bits, seed=500 + d + bits)
    rng = np.random.Generator(np.random.PCG64(7000 + d + bits))
    best = (0.25 * b["prior_scale"] * rng.standard_normal((nb, d))).astype(np.float32)
    return np.stack([b["prior_loc"], b["prior_scale"], b["post_loc"], b["post_scale"], best],
                    axis=2).astype(np.float32)


def _special(d=32):
    """Blocks the header must refuse, with the tile size each is run at."""
    base = _consts(d, 16, 1)[0]
    out = []
    a0 = base.copy(); a0[:, 1] = 0.0                      # alpha = 0 everywhere
    out.append(("alpha0", a0, 1 << 16))
    nn = base.copy(); nn[d // 2, 2] = np.float32("nan")   # a NaN constant
    out.append(("nan", nn, 1 << 16))
    ii = base.copy(); ii[3, 0] = np.float32("inf")        # an inf constant
    out.append(("inf", ii, 1 << 16))
    for e in (40, -40):                                   # sigma scaled by 2^+-40
        s = base.copy(); s[:, 3] *= np.float32(2.0 ** e)
        out.append((f"sigma2^{e}", s, 1 << 16))
    for n in (16, 256):                                   # small tiles
        out.append((f"N{n}", base.copy(), n))
    return out


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """{case: (q [nb, 2], alpha [nb, 2, d], beta [nb, 2, d])}, m; one compile, one run."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "the tau guess check needs a host C++ compiler"
    tmp = tmp_path_factory.mktemp("tau_guess")
    exe, inp = str(tmp / "tau_guess_check"), str(tmp / "in.bin")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", exe,
                           os.path.join(REPO, "tests", "native", "tau_guess_check.cpp")])
    sections = [((d, bits, nb), _consts(d, bits, nb), 1 << bits) for d, bits, nb in CASES]
    sections += [(name, blk[None], n) for name, blk, n in _special()]
    with open(inp, "wb") as f:
        for _, c, n in sections:
            np.array([c.shape[0], c.shape[1], n], np.int64).tofile(f)
            c.tofile(f)
    p = subprocess.run([exe, inp], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout[-2000:]
    lines = p.stdout.split("\n")
    assert lines[0].startswith("m ") and lines[-2:] == ["ok", ""], (lines[0], lines[-3:])
    m = int(lines[0].split()[1])
    out, at = {}, 1
    for key, c, _ in sections:
        nb, d = c.shape[:2]
        a = np.array([[float(x) for x in ln.split()] for ln in lines[at:at + 2 * nb]])
        at += 2 * nb
        a = a.reshape(nb, 2, 1 + 2 * d)
        out[key] = (a[:, :, 0], a[:, :, 1:1 + d], a[:, :, 1 + d:])
    assert at == len(lines) - 2
    return out, m


_erfc = np.vectorize(math.erfc)


def lr_tail(al, be, t):
    """(P, q): Lugannani-Rice P(Q <= K'(t)) and q = K'(t); al, be [..., d], t [...] < 0."""
    w, b2, t = al * al, be * be, t[..., None]
    den = 1.0 - 2.0 * t * w
    k = np.sum(-0.5 * np.log(den) + t * b2 / den, axis=-1)
    k1 = np.sum(w / den + b2 / den ** 2, axis=-1)
    k2 = np.sum(2.0 * w * w / den ** 2 + 4.0 * w * b2 / den ** 3, axis=-1)
    t = t[..., 0]
    r = -np.sqrt(2.0 * (t * k1 - k))
    u = t * np.sqrt(k2)
    p = 0.5 * _erfc(-r / math.sqrt(2.0)) + np.exp(-0.5 * r * r) / math.sqrt(2 * math.pi) * \
        (1.0 / r - 1.0 / u)
    return p, k1


def q_reference(al, be, p0):
    """q_m in float64: bisection on x = ln(-t); P falls as x grows."""
    lo = np.full(al.shape[:-1], -12.0)
    hi = np.full(al.shape[:-1], 12.0)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        p, _ = lr_tail(al, be, -np.exp(mid))
        big = p > p0
        lo = np.where(big, mid, lo)
        hi = np.where(big, hi, mid)
    return lr_tail(al, be, -np.exp(0.5 * (lo + hi)))[1]


def test_kept_m(run):
    _, m = run
    assert m in (4, 6, 8, 12, 16)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "d%d_b%d_nb%d" % c)
def test_q_matches_float64_formula(run, case):
    out, m = run
    q, al, be = out[case]
    d, bits, nb = case
    if m / 2.0 ** bits > 2.0 ** -9:   # the header refuses such tiles
        assert (q == -1.0).all()
        return
    assert (q > 0).all(), f"no guess for {np.count_nonzero(q <= 0)} of {q.size}"
    want = q_reference(al, be, m / 2.0 ** bits)
    rel = np.abs(q - want) / want
    print(f"{case}: max relative difference {rel.max():.3g}")
    assert rel.max() <= Q_RTOL, (rel.max(), np.unravel_index(rel.argmax(), rel.shape))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "d%d_b%d_nb%d" % c)
def test_calibration_monte_carlo(run, case):
    """Rows with Q <= q_m among N = 2^bits rows of numpy normals: m on average
    (within 20%), and at most 1% of the blocks have none."""
    out, m = run
    q, al, be = out[case]
    d, bits, nb = case
    if m / 2.0 ** bits > 2.0 ** -9:   # the header refuses such tiles
        assert (q == -1.0).all()
        return
    rng = np.random.Generator(np.random.PCG64(9000 + d + bits))
    n = 1 << bits
    cnt = np.zeros(nb, np.int64)
    a32, b32 = al[:, 0].astype(np.float32), be[:, 0].astype(np.float32)
    for g in range(nb):
        z = rng.standard_normal((n, d), dtype=np.float32)
        z *= a32[g]
        z += b32[g]
        np.square(z, out=z)
        cnt[g] = np.count_nonzero(z.sum(axis=1, dtype=np.float64) <= q[g, 0])
    print(f"{case}: mean count {cnt.mean():.3f} (m = {m}), blocks with none "
          f"{np.count_nonzero(cnt == 0)} of {nb}")
    assert 0.8 * m <= cnt.mean() <= 1.2 * m, cnt.mean()
    assert np.count_nonzero(cnt == 0) <= 0.01 * nb


def test_no_guess(run):
    out, _ = run
    for name, _, _ in _special():
        q = out[name][0]
        assert (q[:, 0] == -1.0).all(), (name, q)
    # the later step's constants (beta shifted by a finite `best`) of the blocks
    # refused for their alpha or their N: refused as well
    for name in ("alpha0", "sigma2^40", "sigma2^-40", "N16", "N256"):
        assert (out[name][0][:, 1] == -1.0).all(), name
