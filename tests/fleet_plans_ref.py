"""Exchanged plans: what usvmpc_<kind>_fleet_plans and usvmpc_<kind>_fleet_plan_state refuse, word for word and in the entry point's order,
written out by hand from include/usvmpc.h.  tests/test_world_plan_plans.py holds csrc/world_plan.hpp to it on the CPU,
tests/test_gpu_fleet_plans_refusals.py the library on the device."""
KINDS = ("guidance", "pf")
PLAN_NONE, PLAN_SOLVED, PLAN_SHIFTED = 0, 1, 2

# the order of the entries is the order of the checks
REFUSALS = {
    "guidance": [
        ("model", "guidance_fleet_plans: the guidance front end belongs to usv_model_guidance_ca1"),
        ("reset", "guidance_fleet_plans: usvmpc_guidance_reset must be called first"),
        ("fleet", "guidance_fleet_plans: a world list and a fleet (usvmpc_guidance_fleet) come first"),
        ("N", "guidance_fleet_plans: the horizon has N = 1; a scene-mate's plan needs N >= 2"),
    ],
    "pf": [
        ("model", "the path-following front end (usvmpc_pf_*) belongs to usv_model_pf_ca"),
        ("reset", "pf_fleet_plans: usvmpc_pf_reset, a world list and a fleet (usvmpc_pf_fleet) come first"),   # (one refusal with the missing fleet)
        ("fleet", "pf_fleet_plans: usvmpc_pf_reset, a world list and a fleet (usvmpc_pf_fleet) come first"),
        ("N", "pf_fleet_plans: the horizon has N = 1; a scene-mate's plan needs N >= 2"),
    ],
}

STATE_REFUSALS = {
    "guidance": [
        ("model", "guidance_fleet_plan_state: the guidance front end belongs to usv_model_guidance_ca1"),
        ("reset", "guidance_fleet_plan_state: usvmpc_guidance_reset must be called first"),
    ],
    "pf": [
        ("model", "the path-following front end (usvmpc_pf_*) belongs to usv_model_pf_ca"),
        ("reset", "usvmpc_pf_reset must be called first"),
    ],
}
