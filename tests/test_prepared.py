"""The cache of inference-prepared weight forms (models/networks/prepared.py), on CPU tensors: when a form is served,
when it is rebuilt, and the teardown."""
import torch

from centerpoly_amd.models.networks.prepared import ATTR, prepared, release_inference, release_prepared


class _Counter(object):
    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return self.calls


def _get(owner, tensors, build, extra=(), slot="w"):
    return prepared(owner, slot, tensors, build, extra)


def test_same_tensor_builds_once():
    owner, t, build = torch.nn.Module(), torch.randn(4, 3), _Counter()
    assert _get(owner, (t,), build) == (1, True)
    assert _get(owner, (t,), build) == (1, False)
    assert _get(owner, (t,), build) == (1, False)
    assert build.calls == 1


def test_in_place_op_rebuilds():
    owner, t, build = torch.nn.Module(), torch.randn(4, 3), _Counter()
    _get(owner, (t,), build)
    t.mul_(2)
    assert _get(owner, (t,), build) == (2, True)


def test_data_swap_rebuilds():
    """`t.data = u` re-points the storage without a version bump."""
    owner, t, build = torch.nn.Module(), torch.nn.Parameter(torch.randn(4, 3)), _Counter()
    _get(owner, (t,), build)
    version = t._version
    t.data = torch.randn(4, 3)
    assert t._version == version                     # (what the version alone would not see)
    assert _get(owner, (t,), build) == (2, True)


def test_module_to_float64_rebuilds():
    conv, build = torch.nn.Conv2d(3, 4, 3), _Counter()
    w = conv.weight
    _get(conv, (w,), build)
    conv.to(torch.float64)
    assert conv.weight is w                          # same object, new storage
    assert _get(conv, (conv.weight,), build) == (2, True)


def test_other_object_with_equal_values_rebuilds():
    owner, t, build = torch.nn.Module(), torch.randn(4, 3), _Counter()
    _get(owner, (t,), build)
    assert _get(owner, (t.clone(),), build) == (2, True)


def test_extra_change_rebuilds():
    owner, t, build = torch.nn.Module(), torch.randn(4, 3), _Counter()
    _get(owner, (t,), build, extra=(1, (2, 3)))
    assert _get(owner, (t,), build, extra=(1, (2, 3))) == (1, False)
    assert _get(owner, (t,), build, extra=(2, (2, 3))) == (2, True)


def test_every_tensor_is_checked_and_slots_are_separate():
    owner, a, b, build = torch.nn.Module(), torch.randn(2), torch.randn(3), _Counter()
    _get(owner, (a, b), build)
    b.add_(1)
    assert _get(owner, (a, b), build) == (2, True)
    assert _get(owner, (a, b), build, slot="other") == (3, True)
    assert _get(owner, (a, b), build) == (2, False)


def test_release_prepared_clears_every_submodule():
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.Sequential(torch.nn.Conv2d(4, 4, 1)))
    build = _Counter()
    for m in net.modules():
        _get(m, (torch.ones(1),), build)
    assert all(ATTR in vars(m) for m in net.modules())
    release_prepared(net)
    assert not any(ATTR in vars(m) for m in net.modules())
    conv = net[0]
    assert _get(conv, (conv.weight,), build)[1]      # the next call builds again


def test_release_inference_drops_folded_state():
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.Conv2d(4, 4, 1))
    net[0]._folded = (net[0].weight, net[0].bias)
    net._heads_cat = [(torch.ones(1),)]
    net._inter_folded = [(torch.ones(1),)]
    _get(net[1], (net[1].weight,), _Counter())
    release_inference(net)
    assert net[0]._folded is None and net._heads_cat is None and net._inter_folded is None
    assert not any(ATTR in vars(m) for m in net.modules())
    assert not hasattr(net[1], "_folded")            # (nothing is added where there was nothing)
