"""ESPCN upscale factors other than 2, the parts that need no GPU: the "upscale" key of the JSON model through the C++ host mirror's parser and
shape rules, models.espcn_weights(scale=), and the refusal of models whose factor or channel count cannot be a depth-to-space."""
import json

import numpy as np
import pytest


def _json(tmp_path, net, w, h, name=None):
    from shadernn_amd import models

    return models.write_json(net, w, h, str(tmp_path / ((name or net["name"]) + ".json")))


@pytest.mark.parametrize("r", [3, 4])
def test_graph_summary_follows_the_upscale_key(built, tmp_path, r):
    from shadernn_amd import host, models

    W, H = 96, 40
    net = models.espcn_weights(seed=1, scale=r)
    path = _json(tmp_path, net, W, H)
    sub = json.load(open(path))["Layer_4"]
    assert sub["upscale"] == r and sub["inputPlanes"] == r * r and sub["name"] == "subpixel" and sub["type"] == "Lambda"
    rows = host.graph_summary(path, W, H, 1)  # rows are width, height, channels
    assert [x["dims"] for x in rows] == [(W, H, 1), (W, H, 16), (W, H, 16), (W, H, r * r), (r * W, r * H, 1)]


def test_graph_summary_without_the_key_is_x2(built, tmp_path):
    from shadernn_amd import host, models

    W, H = 50, 34
    path = _json(tmp_path, models.espcn_weights(seed=1), W, H)
    assert "upscale" not in open(path).read()
    assert host.graph_summary(path, W, H, 1)[-1]["dims"] == (2 * W, 2 * H, 1)


def test_scale_2_is_the_net_it_always_was(tmp_path):
    from shadernn_amd import models

    a, b = models.espcn_weights(7), models.espcn_weights(7, scale=2)
    assert a["name"] == b["name"] == "ESPCN_2X" and len(a["layers"]) == len(b["layers"]) == 4
    for la, lb in zip(a["layers"], b["layers"]):
        assert sorted(la) == sorted(lb)
        for k in la:
            if isinstance(la[k], np.ndarray):
                np.testing.assert_array_equal(la[k], lb[k])
            else:
                assert la[k] == lb[k], k
    pa, pb = _json(tmp_path, a, 24, 16, "default"), _json(tmp_path, b, 24, 16, "scale2")
    ta, tb = open(pa, "rb").read(), open(pb, "rb").read()
    assert ta == tb and b"upscale" not in ta


@pytest.mark.parametrize("r", [3, 4, 5])
def test_other_scales_change_only_the_tail(r):
    from shadernn_amd import models

    a, b = models.espcn_weights(3), models.espcn_weights(3, scale=r)
    assert b["name"] == "ESPCN_%dX" % r
    for la, lb in zip(a["layers"][:2], b["layers"][:2]):  # the same RNG stream up to the last convolution
        np.testing.assert_array_equal(la["w"], lb["w"])
        np.testing.assert_array_equal(la["b"], lb["b"])
    assert b["layers"][2]["w"].shape == (r * r, 16, 3, 3) and b["layers"][2]["oc"] == r * r
    assert b["layers"][3] == {"type": "Subpixel", "name": "subpixel", "ic": r * r, "oc": 1, "upscale": r}


@pytest.mark.parametrize("bad", ["channels", "zero", "negative", "fraction", "string"])
def test_a_bad_model_is_refused_not_aborted_on(built, tmp_path, bad):
    from shadernn_amd import host, models

    net = models.espcn_weights(seed=1, scale=3)
    path = _json(tmp_path, net, 20, 12)
    d = json.load(open(path))
    if bad == "channels":  # 9 channels cannot be a depth-to-space(4)
        d["Layer_4"]["upscale"] = 4
    else:
        d["Layer_4"]["upscale"] = {"zero": 0, "negative": -3, "fraction": 2.5, "string": "3"}[bad]
    json.dump(d, open(path, "w"))
    with pytest.raises(ValueError):
        host.graph_summary(path, 20, 12, 1)
    # the process is alive and the library still works
    assert host.graph_summary(_json(tmp_path, net, 20, 12, "good"), 20, 12, 1)[-1]["dims"] == (60, 36, 1)
