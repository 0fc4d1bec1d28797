"""Writes tests/golden/report_golden.npz from matplotlib's own "jet" colour map (run once where matplotlib is installed):

    jet          uint8 [256,4]  (jet(i) * 255).astype(uint8) of the 256 table entries: the truncation depth_colorize applies
    jet_rounded  uint8 [256,4]  floor(jet(i) * 255 + 0.5): what torchvision's save_image makes of the float colours

deblurgs_amd.report.jet_table builds both from the published segment definition; tests/test_report_host.py holds it to
this file.
"""
import os

import numpy as np


def main():
    import matplotlib
    colours = matplotlib.colormaps["jet"](np.arange(256))          # integer input: the table entries themselves
    assert colours.shape == (256, 4) and colours.dtype == np.float64
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "report_golden.npz")
    np.savez(out, jet=(colours * 255).astype(np.uint8), jet_rounded=np.floor(colours * 255 + 0.5).astype(np.uint8))
    print(out)


if __name__ == "__main__":
    main()
