"""CPU checkers of the HIP kernels. TEST INFRASTRUCTURE ONLY: the product never imports anything from here.

oracle_py.py       ctypes face of liboracle.so (hanabi_oracle.c, rule_oracle.c): env, rule agents, Philox, sum tree / PER
learner_oracle.py  numpy float64 restatement of the learner arithmetic (loss, projection, backward, Adam, priorities)
actor_oracle.py    numpy float64 restatement of the actor's forward pass and move selection
thin_forward_oracle.py  what hb_thin_forward must and may write (need / may masks) and the two host formulas that size its launch
replay_oracle.py   trajectory oracle of the replay ring: per-game transition lists and a replayed slot map, float64 n-step returns
"""
