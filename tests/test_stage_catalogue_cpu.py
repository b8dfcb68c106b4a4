"""The names DeviceWorkload.prove_stage_batches goes by (no device): every relation of STAGE_BATCHES is found in exactly one of the two places the batches look a name
up in -- the cycle-domain catalogue's members (jolt_amd.workload.build) or the stage operators' table (DeviceExtended.OPERATORS) -- and the table holds no operator
that no stage lists.  The batches themselves: tests/test_gpu_full_stage_batches.py."""
from jolt_amd.stages import DeviceExtended
from jolt_amd.workload import DeviceWorkload, build


def test_every_relation_of_a_stage_batch_is_a_catalogue_member_or_a_stage_operator_never_both():
    _, members, _ = build(4)
    members = {ms.name for ms in members}
    operators = set(DeviceExtended.OPERATORS)
    for key, names in DeviceWorkload.STAGE_BATCHES.items():
        for name in names:
            assert (name in members) != (name in operators), (key, name)
    listed = [name for names in DeviceWorkload.STAGE_BATCHES.values() for name in names if name in operators]
    assert sorted(listed) == sorted(operators - {"spartan_outer"})  # each in exactly one stage; stage 1 (the Spartan outer relation alone) is no batch
    assert set(DeviceWorkload.STAGE_BATCH_LABELS) == set(DeviceWorkload.STAGE_BATCHES)
    assert set(DeviceExtended.HELD_CLAIMS) <= operators
