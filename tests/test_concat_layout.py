"""layers.ConcatLayout -- the one statement of the concat buffer's column layout ``[r_K | r_0 | ... | r_{K-1}]``."""
import pytest
import torch

from h2gcn_amd.layers import ConcatLayout, concat_layout


@pytest.mark.parametrize("K", (1, 2, 3))
@pytest.mark.parametrize("H", (1, 2, 3))
@pytest.mark.parametrize("w0", (1, 6))
def test_concat_layout(w0, H, K):
    lay = ConcatLayout(w0, H, K)
    assert list(lay.widths) == [w0 * H ** k for k in range(K + 1)]
    assert lay.total == w0 * sum(H ** k for k in range(K + 1))
    # the order r_K, r_0, ..., r_{K-1}: each slot starts where the previous one of that order ends
    order = [K] + list(range(K))
    pos = 0
    for k in order:
        assert lay.offsets[k] == pos, (k, lay.offsets)
        pos += lay.widths[k]
    assert pos == lay.total
    with pytest.raises(Exception):   # immutable ...
        lay.total = 0
    assert concat_layout(w0, H, K) == lay and concat_layout(w0, H, K) is concat_layout(w0, H, K)   # ... hence shared

    n = 5
    t = torch.arange(n * lay.total, dtype=torch.float32).reshape(n, lay.total)
    item = t.element_size()
    for k in range(K + 1):
        s = lay.slot(t, k)
        assert s.shape == (n, lay.widths[k])
        assert s.data_ptr() == t.data_ptr() + lay.offsets[k] * item and s.stride() == (lay.total, 1)   # a view: no copy
        assert torch.equal(s, t[:, lay.offsets[k]:lay.offsets[k] + lay.widths[k]])
        if k == 0:
            continue
        v = lay.hop_view(t, k)
        assert v.shape == (n, H, lay.widths[k - 1])
        assert v.data_ptr() == s.data_ptr() and v.stride() == (lay.total, lay.widths[k - 1], 1)
        assert torch.equal(v.reshape(n, lay.widths[k]), s)                       # hop h of round k = columns h*w .. (h+1)*w of the slot
        assert torch.equal(lay.hops(s, k), v) and lay.hops(s, k).data_ptr() == s.data_ptr()
    assert torch.equal(torch.cat([lay.slot(t, k) for k in order], dim=1), t)
    assert torch.equal(torch.cat([lay.slot(t, 0)] + [lay.hop_view(t, k).flatten(1) for k in range(1, K + 1)], dim=1),
                       torch.cat([lay.slot(t, k) for k in range(K + 1)], dim=1))
