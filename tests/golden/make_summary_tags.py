"""Writes tests/golden/summary_tags.json: the input names of the four MergeSummary nodes of the reference's graph
(training.py:144-149), in input order -- the tags TensorBoard shows for a run of the reference.

    python tests/golden/make_summary_tags.py <reference>/model/air-model.meta

Merge: 88 ScalarSummary (test model), Merge_1: 36 HistogramSummary, Merge_2: 1 ImageSummary, Merge_3: 216 gradient
summaries of the train model (histogram, norm, average per gradient, original then applied).  A summary node's name IS its
tag for these (tf.summary.* names the node after the tag; the ':0' of a variable's name becomes '_0')."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle.graphdef_pin import load_nodes  # noqa: E402

MERGES = (("numeric", "Merge/MergeSummary", "ScalarSummary", 88), ("variables", "Merge_1/MergeSummary", "HistogramSummary", 36),
          ("image", "Merge_2/MergeSummary", "ImageSummary", 1), ("gradients", "Merge_3/MergeSummary", None, 216))


def main(meta, out=os.path.join(HERE, "summary_tags.json")):
    _, nodes = load_nodes(meta)
    tags = {}
    for key, node, op, count in MERGES:
        names = [i.split(":")[0] for i in nodes[node]["inputs"]]
        assert len(names) == count, (node, len(names))
        ops = {nodes[n]["op"] for n in names}
        assert ops == ({op} if op else {"HistogramSummary", "ScalarSummary"}), (node, ops)
        tags[key] = names
    with open(out, "w") as f:
        json.dump(tags, f, indent=0)
        f.write("\n")
    return tags


if __name__ == "__main__":
    main(sys.argv[1])
