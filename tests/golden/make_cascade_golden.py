"""Writes tests/golden/cascade_skimage.npz: what scikit-image 0.18.3 (skimage.feature.Cascade, an evaluator independent of
this repository) finds with the OpenCV-trained LBP model it ships, tests/golden/lbpcascade_frontalface_opencv.xml (a copy of
skimage/data/lbpcascade_frontalface_opencv.xml; model data, distributed with scikit-image under its BSD-3-Clause licence,
trained with OpenCV's traincascade).  Run with a Python that has scikit-image 0.18.3 and Pillow:

    python tests/golden/make_cascade_golden.py

Holds: the 256 x 256 gray face crop astronaut()[0:256, 100:356] (skimage.color.rgb2gray, times 255, rounded); the crop
resized to 72, 80 and 88 pixels with Pillow's bilinear filter (the planes themselves, as bytes); per plane the scale-1 windows (row, col) that pass every stage, asked for with arguments that stop
scikit-image from merging detections; scikit-image's own multi-scale box for the crop."""
import os

import numpy as np
import skimage
from PIL import Image
from skimage import data
from skimage.color import rgb2gray
from skimage.feature import Cascade

HERE = os.path.dirname(os.path.abspath(__file__))
SIDES = (72, 80, 88)


def main():
    assert skimage.__version__ == "0.18.3", skimage.__version__
    det = Cascade(os.path.join(HERE, "lbpcascade_frontalface_opencv.xml"))
    crop = np.round(rgb2gray(data.astronaut()[0:256, 100:356]) * 255).astype(np.uint8)
    out = {"crop": crop}
    for side in SIDES:
        plane = np.asarray(Image.fromarray(crop).resize((side, side), Image.BILINEAR), dtype=np.uint8)
        found = det.detect_multi_scale(img=plane, scale_factor=1.2, step_ratio=1, min_size=(24, 24), max_size=(25, 25),
                                       min_neighbour_number=1, intersection_score_threshold=2.0)
        assert all(d["width"] == 24 and d["height"] == 24 for d in found), found
        wins = sorted((int(d["r"]), int(d["c"])) for d in found)
        assert len(wins) >= 1, f"no raw window on the {side}-pixel plane"
        assert len(set(wins)) == len(wins), f"equal windows on the {side}-pixel plane: a merge happened"
        print(side, wins)
        out[f"plane{side}"] = plane
        out[f"windows{side}"] = np.array(wins, dtype=np.int32).reshape(-1, 2)
    box = det.detect_multi_scale(img=crop, scale_factor=1.2, step_ratio=1, min_size=(60, 60), max_size=(123, 123))
    assert len(box) == 1, box
    out["multiscale_box"] = np.array([box[0]["r"], box[0]["c"], box[0]["width"], box[0]["height"]], dtype=np.int32)   # r, c, w, h
    print("multi-scale", out["multiscale_box"])
    np.savez_compressed(os.path.join(HERE, "cascade_skimage.npz"), **out)


if __name__ == "__main__":
    main()
