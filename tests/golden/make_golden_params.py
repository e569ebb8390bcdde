"""Generates tests/golden/benchmark_params.json: the FollowPath section (optimizer block with its weights, trajectorizer
block) of the reference's three shipped parameter files, as values, so that tests/test_host.py can check the parameter
presets against them without the reference tree:

    python tests/golden/make_golden_params.py <reference>/params

Only the section OptimizerParams.from_yaml reads is kept; the rest of each file (navigator, costmaps, servers) is not."""
import json
import os
import sys

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = ("soc_work_obst_parameters_in_benchmark.yaml", "obst_only_parameters_in_benchmark.yaml", "params.yaml")


def follow_path(node, plugin="FollowPath"):
    if isinstance(node, dict):
        if plugin in node and isinstance(node[plugin], dict) and "optimizer" in node[plugin]:
            return node[plugin]
        for v in node.values():
            r = follow_path(v, plugin)
            if r is not None:
                return r
    return None


def main(src):
    out = {}
    for name in FILES:
        with open(os.path.join(src, name)) as f:
            sec = follow_path(yaml.load(f, Loader=yaml.SafeLoader))
        out[name] = {"optimizer": sec["optimizer"], "trajectorizer": sec["trajectorizer"]}
    with open(os.path.join(HERE, "benchmark_params.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
