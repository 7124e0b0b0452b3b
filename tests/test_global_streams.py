"""Global agent ids, host side: the shard recipe partitions a population exactly (no GPU needed)."""
import pytest

from visfly_amd import parallel


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n_total", [8, 512, 513, 1000, 262144 + 5])
def test_shard_kwargs_partitions_exactly(world, n_total):
    kws = [parallel.shard_kwargs(n_total, rank=r, world=world) for r in range(world)]
    assert all(set(k) == {"num_agent_per_scene", "agent_offset"} for k in kws)
    nxt = 0
    for k in kws:                                   # contiguous, in rank order, nobody empty
        assert k["agent_offset"] == nxt and k["num_agent_per_scene"] >= 1
        nxt += k["num_agent_per_scene"]
    assert nxt == n_total
    counts = [k["num_agent_per_scene"] for k in kws]
    assert max(counts) - min(counts) <= 1           # remainders spread one apiece
    assert [(k["agent_offset"], k["num_agent_per_scene"]) for k in kws] == [parallel.shard(n_total, r, world) for r in range(world)]


def test_shard_kwargs_defaults_to_the_process_group():
    assert parallel.shard_kwargs(77) == dict(num_agent_per_scene=77, agent_offset=0)      # no process group: world 1, rank 0


def test_shard_kwargs_refuses_bad_ranks_and_empty_shards():
    with pytest.raises(ValueError):
        parallel.shard_kwargs(16, rank=2, world=2)
    with pytest.raises(ValueError):
        parallel.shard_kwargs(16, rank=-1, world=2)
    with pytest.raises(ValueError):
        parallel.shard_kwargs(2, rank=2, world=3)


def test_new_entry_points_have_signatures():
    from visfly_amd import _lib
    for s in ("vf_env_set_agent_offset", "vf_env_agent_offset", "vf_head_sample_at", "vf_noise_fill"):
        assert s in _lib.SIGNATURES
