"""Writes tests/golden/jpeg_decode_golden.npz: for every case of tests/jpeg_decode_cases.py the .jpg file Pillow
(libjpeg-turbo) makes of the case's image and the pixels Pillow decodes from it.  Run from the repository root:

    python tests/golden/make_golden_jpeg_decode.py

The fixtures were made with Pillow 12.2.0.  Every case's preconditions are asserted on the file before it is stored, and
the restatement must already equal Pillow's pixels: a fixture that the specification does not explain is not written.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_decode_cases as dc  # noqa: E402


def main():
    dc.check_table()
    arrays = {}
    for name in dc.CASES:
        data, pixels = dc.pillow_file(name)
        dc.check_needs(name, data)
        assert np.array_equal(dc.decode(data), pixels), name
        arrays[f"file/{name}"] = np.frombuffer(data, dtype=np.uint8)
        arrays[f"pixels/{name}"] = pixels
    np.savez_compressed(dc.GOLDEN, **arrays)
    print(f"{dc.GOLDEN}: {len(dc.CASES)} cases, {os.path.getsize(dc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
