"""The references of tests/heads_ref.py checked on the host, before any kernel is held to
them: the restated Philox4x32-10 rounds against the Random123 known answers, the counter
arithmetic of the restated sampler, and the float32-vs-float64 figures the GPU gates of
tests/test_gpu_direct_calls.py are derived from.  No GPU."""
import numpy as np

import heads_ref as H


def words(out):
    return " ".join("%08x" % int(w[0]) for w in out)


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    assert words(H.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert words(H.philox4x32_10((ones,) * 4, (ones,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert words(H.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344),
                                 (0xA4093822, 0x299F31D0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_restated_sampler_counter_arithmetic():
    """offset = k skips 4 k draws; the 64-bit counter carries from its low word into its high
    word (offset 2^32 - 2 + i) and wraps at 2^64; the four draws of a counter are the Box-Muller
    pairs of (c0, c1) and (c2, c3)."""
    seed = 2 ** 40 + 3
    assert np.array_equal(H.normal_ref(1027, seed, 3), H.normal_ref(1027 + 12, seed, 0)[12:])
    a = H.normal_ref(16, seed, 2 ** 32 - 2)
    assert np.array_equal(a[8:], H.normal_ref(8, seed, 2 ** 32))
    assert not np.array_equal(a[8:], H.normal_ref(8, seed, 0))       # the carry is not dropped
    w = H.normal_ref(8, seed, 2 ** 64 - 1)
    assert np.array_equal(w[4:], H.normal_ref(4, seed, 0))
    c = [float(v[0]) for v in H.philox4x32_10((5, 0, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))]
    u = [(v + 0.5) * 2.0 ** -32 for v in c]
    r0, r1 = np.sqrt(-2 * np.log(u[0])), np.sqrt(-2 * np.log(u[2]))
    want = [r0 * np.cos(2 * np.pi * u[1]), r0 * np.sin(2 * np.pi * u[1]),
            r1 * np.cos(2 * np.pi * u[3]), r1 * np.sin(2 * np.pi * u[3])]
    assert np.allclose(H.normal_ref(4, seed, 5), want, rtol=0, atol=1e-14)
    for n in (1, 2, 3, 5):
        assert np.array_equal(H.normal_ref(n, seed, 7), H.normal_ref(8, seed, 7)[:n])


def test_float32_restatement_figures_behind_the_gpu_gates():
    """What float32 costs against the float64 references, on one of the sampler's draws (the one
    with the largest deviation of the 16 the GPU test runs: 4.31e-5, 99.9 % within 1.05e-6) and
    on the small Adam cases (the largest over all: 3.7e-7, late-steps)."""
    n, seed, offset = 2 ** 20 + 3, 1234, 2 ** 32 - 2
    d = np.abs(H.normal_ref(n, seed, offset, np.float32).astype(np.float64) - H.normal_ref(n, seed, offset))
    assert 4.2e-5 < d.max() < 4.4e-5 and np.quantile(d, 0.999) < 1.05e-6
    worst = max(H.adam_deviation(c, H.adam_run(c, np.float32))
                for c in map(H.adam_case, ("one", "late-steps", "late-steps-amsgrad", "wide-range")))
    assert 3.0e-7 < worst < 3.7e-7


def test_heads_cases_hit_what_they_were_chosen_for():
    """The planning port on the shape family: the launch properties the cases' comments name."""
    P, X = H.partial_launch, H.expand_launch
    assert P(1, 16, 4, 2)[1:] == (1, 8512, 1, 64, 16)               # one chunk, NP = 16
    assert P(70, 16, 1, 6)[0] == 16 and P(70, 16, 1, 6)[3] == 1     # KS = 1, 5 tiles of 16
    assert P(3, 32, 16, 20)[5] == 32                                 # N = 20 in NP = 32
    assert P(37, 64, 9, 40)[4:] == (72, 64)                          # KC = 72
    assert X(5, 256, 1, 7)[:2] == (1, 1) and H.heads_cc(256, 1) == 128
    assert P(129, 256, 9, 18)[1] == 2 and X(129, 256, 9, 9)[1] == 4
    assert P(300, 256, 4, 128)[1] == 4 and X(300, 256, 4, 128)[2] == 133120
    assert P(9, 16, 256, 128)[2:5] == (134152, 16, 256) and X(9, 16, 256, 64)[1] == 8
    assert P(4, 64, 144, 48)[3:5] == (64, 144)
    assert P(700, 16, 9, 80)[5] == 128 and P(700, 16, 9, 80)[0] == 4     # 175 tiles of 4
    assert P(2000, 32, 4, 128)[1:4:2] == (2, 1)
    assert P(4, 16, 289, 128)[2] == 151444 and P(4, 16, 324, 128)[2] > H.LDS_MAX
    assert all(H.heads_shape_ok(B, C, S, L) for C, S, L, B in H.HEADS_CASES + H.PLAN_SHAPES)
    assert not any(H.heads_shape_ok(*s) for s in H.REFUSED)
