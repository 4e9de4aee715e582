"""The lifecycle the handle classes on voxel_slam_amd.vxba's shared base have in common (create, ``with``, close, close again) on device 0 with
no data pushed, and the one class whose close differs: a ``LoopSearch`` that outlives its ``LoopRegistration``.  No entry point is called on a
closed handle."""
import pytest

pytestmark = pytest.mark.gpu


def test_every_class_on_the_shared_base_opens_and_closes_the_same_way():
    import contextlib
    import ctypes as C
    from voxel_slam_amd import vxba
    names = ("LioEstimator", "InitOdometry", "ImuEkf", "PoseGraph", "LoopRegistration", "LoopSearch", "LocalMap", "KeyframeBuilder", "CornerExtractor")
    for name in names:
        with contextlib.ExitStack() as stack:          # closes a LoopSearch's registration after the search itself
            obj = vxba.LoopSearch(stack.enter_context(vxba.LoopRegistration())) if name == "LoopSearch" else getattr(vxba, name)()
            assert isinstance(obj, vxba._Handle) and isinstance(obj._h, C.c_void_p) and obj._h.value, name
            with obj as entered:
                assert entered is obj and obj._h.value, name
            assert not obj._h, name
            obj.close()
            obj.close()
            assert not obj._h and obj._chk is not None and obj._L is vxba.load_library(), name


def test_a_loop_search_follows_its_registration():
    from voxel_slam_amd import vxba
    reg = vxba.LoopRegistration()
    search = vxba.LoopSearch(reg)
    assert search.num_frames() == 0
    reg.close()                                        # takes the stream the search handle shares with it
    search.close()                                     # ... so there is nothing left to destroy, and nothing raises
    search.close()
    assert not search._h and not reg._h
    with vxba.LoopRegistration() as live:
        with pytest.raises(vxba.VxbaError, match="VXBA_ERR_"):
            vxba.LoopSearch(live, device=4096)
        assert live.num_clouds() == 0                  # the registration is untouched by the failed create
