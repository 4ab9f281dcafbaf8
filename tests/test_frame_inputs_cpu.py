"""muggled_dpt_amd/frame_inputs.py is pure host code: the crop rule, the argument checks and the chunk plans of the uint8 frame routes need neither
the native binding nor a device, and DPTModel's module hands out the very same functions under the names callers already import."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frame_inputs_loads_without_the_native_binding():
    """In a fresh process, from its file: the package's __init__ imports DPTModel (and with it the binding), so the module is loaded on its own -
    a relative import of anything in the package would fail here too."""
    code = ("import importlib.util, sys\n"
            "spec = importlib.util.spec_from_file_location('frame_inputs', sys.argv[1])\n"
            "m = importlib.util.module_from_spec(spec)\n"
            "spec.loader.exec_module(m)\n"
            "assert 'muggled_dpt_amd.native' not in sys.modules and 'muggled_dpt_amd' not in sys.modules, sorted(k for k in sys.modules if 'mdpt' in k or 'muggled' in k)\n"
            "assert m.image_chunks([(4, 6), (8, 8), (4, 6), (4, 6)], lambda h, w: (2 * h, 2 * w), 2) == [((8, 12), [0, 2]), ((8, 12), [3]), ((16, 16), [1])]\n"
            "assert m.region_chunks([(0, 1, 2, 7, 6), (1, 0, 0, 6, 4)], lambda h, w: (h, w), 8) == [((4, 6), [0, 1])]\n"
            "assert m._crop_box((40, 60), (slice(-10, None), slice(None, -7))) == (0, 30, 53, 40)\n"
            "assert m.crop_slices_from_norm((100, 100), ((0.125, 0.125), (0.375, 0.375))) == (slice(12, 38), slice(12, 38))\n"
            "print('HOST_ONLY_OK')\n")
    r = subprocess.run([sys.executable, "-c", code, os.path.join(REPO, "muggled_dpt_amd", "frame_inputs.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "HOST_ONLY_OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


def test_dpt_model_and_the_package_hand_out_the_same_functions():
    import muggled_dpt_amd
    from muggled_dpt_amd import dpt_model, frame_inputs
    for name in ("crop_slices_from_norm", "is_cropping", "_is_crop", "_crop_box", "_crop_host", "_row_pitch", "_in_place", "_check_frames", "_check_images",
                 "_check_crops", "_check_regions", "image_chunks", "region_chunks"):
        assert getattr(dpt_model, name) is getattr(frame_inputs, name), name
    assert muggled_dpt_amd.crop_slices_from_norm is frame_inputs.crop_slices_from_norm and muggled_dpt_amd.is_cropping is frame_inputs.is_cropping
