"""Write tests/golden/rejection_sampler_cases.npz: the numbers of the reference's
RejectionSamplerTest.Basic and .Mask (src/speculative/rejection_sampler_test.cpp:14-85), as data only.

    python tests/golden/make_rejection_golden.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    cases = dict(
        # Basic: one sequence, k = 3, vocab 5; the given uniforms accept rows [1, 1, 0]
        basic_draft_token_ids=np.array([[1, 2, 3]], np.int32),
        basic_draft_probs=np.array([[[0.2104, 0.2163, 0.1912, 0.1937, 0.1884],
                                     [0.2100, 0.1803, 0.2398, 0.2088, 0.1610],
                                     [0.1838, 0.2079, 0.2270, 0.2451, 0.1362]]], np.float32),
        basic_target_probs=np.array([[[0.1299, 0.2462, 0.1821, 0.1354, 0.3064],
                                      [0.1159, 0.2839, 0.1603, 0.2451, 0.1949],
                                      [0.0002, 0.0433, 0.6629, 0.1469, 0.1467]]], np.float32),
        basic_uniform=np.array([[0.4785, 0.6589, 0.9399]], np.float32),
        basic_bonus_token_ids=np.array([5], np.int32),
        basic_accepted=np.array([[1, 1, 0]], bool),
        basic_expected_output=np.array([[1, 2, 2, 5]], np.int32),
        basic_expected_masked=np.array([[1, 2, 2, -1]], np.int32),
        # Mask: accepted matrix -> mask up to and including the first rejection
        mask_accepted=np.array([[0, 1, 0, 1], [1, 0, 1, 1], [1, 1, 0, 1], [1, 1, 1, 1]], bool),
        mask_expected=np.array([[1, 0, 0, 0, 0], [1, 1, 0, 0, 0], [1, 1, 1, 0, 0], [1, 1, 1, 1, 1]], bool),
    )
    np.savez(os.path.join(HERE, "rejection_sampler_cases.npz"), **cases)


if __name__ == "__main__":
    main()
