# tests/cpp/attention_bwd_half_sim.mk — TEST CODE: the one rule of attention_bwd_half_sim, beside tests/cpp/Makefile (which it
# includes for CXX, CSRC, SIM_SAN, SIM_HDRS and sanitizer_probe), as attention_bwd_sim.mk.
#   attention_bwd_half_sim   csrc/attention_bwd.hip (with attention_bwd_half_kernel.hpp and attention_bwd_slice_walk.inc)
#                            compiled UNCHANGED with the host compiler over simt/, with the address and undefined-behaviour
#                            sanitizers, beside csrc/coo_csr.hip compiled the same way (the transpose that a create runs),
#                            and driven through mi355_spmv_attention_bwd_create_half / _set_scale / _execute / _destroy: the
#                            program of tests/test_attention_bwd_half_sim_cpu.py, built on demand by it:
#                                make -C tests/cpp -f attention_bwd_half_sim.mk attention_bwd_half_sim
include Makefile

attention_bwd_half_sim: attention_bwd_half_sim.cpp sim_runtime.hpp $(CSRC)/attention_bwd.hip $(CSRC)/attention_bwd_half_kernel.hpp $(CSRC)/attention_bwd_slice_walk.inc $(CSRC)/coo_csr.hip $(SIM_HDRS)
	$(CXX) -std=c++17 -O1 -g -fno-omit-frame-pointer $(SIM_SAN) -Isimt -o $@ $<
