"""child process of test_gpu_range_guard.py: the kernel switches (TRAJSDE_NODE_FP32) and TRAJSDE_LIB
are read once per process, so the cells of the site x route table that depend on them run here.  `cells SITE ...`: the `infer` (and
`exact`) cell of each site under the forms the environment selects; `strict V ...`: every site's plant at the magnitudes V through the
bf16x6 library TRAJSDE_LIB names.  Prints the "[range-guard]" lines of the cells and one JSON verdict line; an assertion that fails ends
the process with its traceback."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(os.path.dirname(HERE), "oracle")]


def main():
    import test_gpu_range_guard as R
    what, args = sys.argv[1], sys.argv[2:]
    ratios = R.strict_cells([float(a) for a in args]) if what == "strict" else R.child_cells(args)
    print(json.dumps({"ok": True, "what": what, "fp16x3": R.fp16x3(), "ratios": ratios}))


if __name__ == "__main__":
    main()
