 Eb,Uk*7BD.TXz
ERcrez]ĩl["McI2ýNe0l-03+bI$)T%Rh"E}W{O}#/we D\|<]ĉ@>?HS09p"(~\ NWZxt?wws5!-.Acu"NKfb:QbY[LK-_8ܶZ#e{ h8My#EmӛkjD4mVVבO#%qϫCY*htNw