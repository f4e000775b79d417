"""Case tuples of the 64-vertex decode fixtures, shared by gen_decode_wide_golden.py and tests/test_wide_polygons.py.
Inputs regenerate from cases.decode_inputs_np (synth streams named after the case)."""

WIDE_DECODE_CASES = [
    # name, B, C, h, w, N, K, rep
    ("cart64", 1, 8, 32, 64, 64, 128, "cartesian"),
    ("polar64", 1, 8, 32, 64, 64, 128, "polar"),
]
