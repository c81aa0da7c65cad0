"""Disparity evaluation (temporalstereo_amd/evaluation.py): the reference's corner cases and the paths that return before any
launch, and the C ABI's workspace query -- no GPU needed."""
import warnings

import pytest
import torch

from temporalstereo_amd import evaluation as ev

KEYS = ['1px', '2px', '3px', '5px', 'epe']


def _is_zero_dict(d, prefix=''):
    assert sorted(d) == sorted(prefix + k for k in KEYS)
    for v in d.values():
        assert v.shape == (1,) and v.dtype == torch.float32 and float(v) == 0.0


def test_none_inputs_warn_and_return_empty():
    x = torch.zeros(1, 1, 4, 4)
    for call in (lambda: ev.do_evaluation(None, x, 0, 192), lambda: ev.do_evaluation(x, None, 0, 192),
                 lambda: ev.do_occlusion_evaluation(None, x, x, 0, 192), lambda: ev.do_occlusion_evaluation(x, None, x, 0, 192),
                 lambda: ev.do_occlusion_evaluation(x, x, None, 0, 192)):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            assert call() == {}
        assert len(w) == 1 and "None" in str(w[0].message)


def test_non_tensor_inputs_give_the_zero_dict():
    _is_zero_dict(ev.calc_error())
    _is_zero_dict(ev.calc_error([1.0, 2.0], torch.zeros(2)))
    _is_zero_dict(ev.do_evaluation(1.0, 2.0, 0, 192))
    d = ev.do_occlusion_evaluation([[1.0]], [[1.0]], [[1.0]], 0, 192)
    _is_zero_dict({k: v for k, v in d.items() if k.startswith('occ_')}, 'occ_')
    _is_zero_dict({k: v for k, v in d.items() if k.startswith('noc_')}, 'noc_')


def test_validation_metrics_paths_without_launch_and_key_names():
    x = torch.zeros(1, 1, 4, 4)
    assert ev.validation_metrics([x, x], None) == {}
    assert ev.validation_metrics([x, x], x, x, eval_ids=[2, 3, 7]) == {}          # every id filtered out (log_metric :469)
    assert ev.validation_metrics([], x, x) == {}
    assert ev.metric_keys(3, eval_ids=[0, 2, 5], occlusion=False) == \
        ['metric_disparity_0/all_' + k for k in KEYS] + ['metric_disparity_2/all_' + k for k in KEYS]
    keys = ev.metric_keys(2)
    assert len(keys) == 2 * 3 * 5 and keys[:5] == ['metric_disparity_0/all_' + k for k in KEYS]
    assert keys[5:10] == ['metric_disparity_0/occ_' + k for k in KEYS] and keys[10:15] == ['metric_disparity_0/noc_' + k for k in KEYS]
    assert keys[15] == 'metric_disparity_1/all_1px'


def test_cpu_tensors_are_refused():
    x = torch.zeros(1, 1, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.calc_error(x, x, 0, 192)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.validation_metrics([x], x)


def test_workspace_query():
    from temporalstereo_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    assert L.ts_disp_metrics_workspace_bytes(1, 544, 960) > 0
    assert L.ts_disp_metrics_workspace_bytes(4, 64, 128) > 0
    assert L.ts_disp_metrics_workspace_bytes(2, 1, 1) > 0
    assert L.ts_disp_metrics_workspace_bytes(4, 544, 960) % 256 == 0
    for args in ((0, 544, 960), (1, 0, 960), (1, 544, 0), (-1, 4, 4), (65536, 65536, 2)):
        assert L.ts_disp_metrics_workspace_bytes(*args) == 0, args
