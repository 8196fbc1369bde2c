"""Loader for tests/golden/gcn_reference_*.npz -- vectors recorded while the reference's own chem_tensorflow_gcn.py ran
(tests/golden/make_reference_gcn_golden.py).  Nothing here touches the reference itself."""
import json
import os
import pickle

import numpy as np

import reference_golden as RG

CASES = ["default", "bias_h64", "multitask", "h48"]
FEED_KEYS = ("initial_node_representation", "adjacency_list", "adjacency_weights", "graph_nodes_list", "target_values",
             "target_mask", "num_graphs")


def path(case):
    return os.path.join(RG.GOLDEN, "gcn_reference_%s.npz" % case)


class GCNGolden:
    def __init__(self, case):
        z = np.load(path(case), allow_pickle=False)
        self.z, self.case = z, case
        self.params = json.loads(str(z["params"]))
        self.names = [str(n) for n in z["trainable_names"]]
        self.shapes = [tuple(json.loads(str(s))) for s in z["trainable_shapes"]]
        self.train_molecules = json.loads(str(z["train_molecules"]))
        self.valid_molecules = json.loads(str(z["valid_molecules"]))
        self.weights = {n: RG.golden_weights(n, s, int(z["weight_seed"])) for n, s in zip(self.names, self.shapes)}

    def feed(self, prefix):
        return {k: self.z["%s_feed_%s" % (prefix, k)] for k in FEED_KEYS}

    def write_checkpoint(self, path_):
        """The golden weights in the reference's pickle schema (chem_tensorflow.py:309-323)."""
        with open(path_, "wb") as f:
            pickle.dump({"params": self.params, "weights": dict(self.weights), "train_step": 0, "valid_step": 0}, f)
        return path_

    def model_args(self, device, **extra):
        args = {"--quiet": True, "--device": device, "--config": json.dumps(self.params),
                "train_data": self.train_molecules, "valid_data": self.valid_molecules}
        args.update(extra)
        return args


def assert_feed_equal(b, ref):
    for key, r in ref.items():
        x = b[key]
        x = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
        r = np.asarray(r)
        if key == "adjacency_weights":                  # (fed as float64, converted by the float32 placeholder)
            r = r.astype(np.float32)
        assert x.shape == r.shape, (key, x.shape, r.shape)
        np.testing.assert_array_equal(x.astype(np.float64), r.astype(np.float64), err_msg=key)
